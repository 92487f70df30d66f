// deepreadmapper_amd/csrc/contig_hits.hip -- the contig stage of a multi-contig reference, for gfx950.
//
// The step between the SW rerank and everything that consumes its rows (include/drm_hip.h, drm_contig_hits): of a
// read's counted rows keep those whose window [id >> 1, id >> 1 + ref_len) lies wholly inside one contig of the table,
// compact them stably, and emit beside the real ids the spread ids id + (contig << 33) that keep the pair-level kernels
// from ever relating two rows of different contigs.
//
// Mapping: one wave per read, a bounded grid looping over reads with the static r += gridDim.x.
// A read's rows are loaded 64 at a time, one per lane, up to 16 chunks held in registers (the kernel is instantiated for
// 1, 2, 4, 8 and 16 chunks, so that a short list pays for no more); every load is issued before the first search. The
// contig of a row is found by a binary search for the last start <= position, ceil(log2 n) branch-free trips whose
// count the host passes, followed by one test against that contig's end. A table of up to kContigLdsMax contigs is
// staged in LDS once per wave (starts, then ends: 16 bytes a contig); a larger one is searched where it lies, its upper
// levels staying in L2. The compaction is a ballot per chunk: a kept row goes to (rows kept so far) + (kept rows on
// lower lanes), the running count being wave-uniform. Rows from the kept count to k get the fill. Every loop runs to a
// clamped count, nothing waits on data, and the outputs never alias the inputs (the entry points check it).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "drm_device.h"
#include "locus_scan.h"

namespace drm {
namespace {

template <int CH, bool LDS>
__global__ __launch_bounds__(64) void contig_hits_kernel(ContigArgs a)
{
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x;
    const int k = a.k, n = a.n;
    if (LDS) {
        uint64_t *ls = reinterpret_cast<uint64_t *>(smem);
        for (int i = lane; i < n; i += 64) {
            ls[i] = a.starts[i];
            ls[n + i] = a.ends[i];
        }
        __syncthreads(); // the block is one wave: this only orders the wave's own LDS writes before its reads
    }
    const uint64_t *ts = LDS ? reinterpret_cast<const uint64_t *>(smem) : a.starts;
    const uint64_t *te = LDS ? reinterpret_cast<const uint64_t *>(smem) + n : a.ends;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    const uint64_t span = (uint64_t)a.ref_len;

    for (int64_t r = blockIdx.x; r < a.nreads; r += gridDim.x) {
        const int c = __builtin_amdgcn_readfirstlane(min(max(a.cnt[r], 0), k));
        const uint64_t *ids = a.ids + r * k;
        const int32_t *sc = a.scores + r * k;
        uint64_t *oi = a.out_ids + r * k, *os = a.out_spread + r * k;
        int32_t *osc = a.out_scores + r * k, *oc = a.out_contig + r * k;

        uint64_t w[CH];
        int32_t s[CH];
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            const int j = ch * 64 + lane;
            w[ch] = j < c ? ids[j] : 0;
            s[ch] = j < c ? sc[j] : 0;
        }
        int m = 0; // rows kept so far, the same on every lane
#pragma unroll
        for (int ch = 0; ch < CH; ++ch) {
            if (ch * 64 >= c) // wave-uniform
                break;
            const uint64_t p = w[ch] >> 1;
            int lo = 0, hi = n; // the last start <= p lies in [lo, hi), if there is one
            for (int it = 0; it < a.steps; ++it) {
                const int mid = (lo + hi) >> 1; // lo <= mid < n
                const bool le = ts[mid] <= p;
                lo = le ? mid : lo;
                hi = le ? hi : mid;
            }
            const bool keep = ch * 64 + lane < c && ts[lo] <= p && p + span <= te[lo];
            const uint64_t mask = __ballot(keep);
            if (keep) {
                const int at = m + __popcll(mask & below);
                oi[at] = w[ch];
                os[at] = w[ch] + ((uint64_t)lo << 33);
                osc[at] = s[ch];
                oc[at] = lo;
            }
            m += __popcll(mask);
        }
        for (int j = m + lane; j < k; j += 64) {
            oi[j] = ~(uint64_t)0;
            os[j] = ~(uint64_t)0;
            osc[j] = 0;
            oc[j] = -1;
        }
        if (lane == 0)
            a.out_cnt[r] = m;
    }
}

template <int CH> void launch_chunks(const ContigArgs &a, hipStream_t stream)
{
    const bool in_lds = a.n <= kContigLdsMax;
    const size_t lds = in_lds ? (size_t)16 * a.n : 0;
    const int grid = bounded_grid(a.nreads, std::max<size_t>(lds, 64));
    if (in_lds)
        hipLaunchKernelGGL((contig_hits_kernel<CH, true>), dim3(grid), dim3(64), lds, stream, a);
    else
        hipLaunchKernelGGL((contig_hits_kernel<CH, false>), dim3(grid), dim3(64), 0, stream, a);
}

} // namespace

void launch_contig_hits(ContigArgs a, hipStream_t stream)
{
    if (a.nreads <= 0)
        return;
    check_k(a.k, "contig");
    if (a.n < 1 || a.n > (1 << 20))
        throw Error(DRM_ERR_ARG, "a contig table of " + std::to_string(a.n) + " contigs, outside [1, 2^20]");
    a.steps = 0;
    while (((int64_t)1 << a.steps) < a.n)
        ++a.steps;
    const int chunks = (a.k + 63) / 64;
    if (chunks <= 1)
        launch_chunks<1>(a, stream);
    else if (chunks <= 2)
        launch_chunks<2>(a, stream);
    else if (chunks <= 4)
        launch_chunks<4>(a, stream);
    else if (chunks <= 8)
        launch_chunks<8>(a, stream);
    else
        launch_chunks<16>(a, stream);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
