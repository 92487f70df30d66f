// deepreadmapper_amd/csrc/hit_loci.hip -- the list of distinct loci in a read's reranked hit list, for gfx950.
//
// hit_mapq_kernel (mapq.hip) runs the greedy locus scan of a list and keeps the best competitor's score and a count.
// This kernel runs the same scan and keeps the loci themselves (include/drm_hip.h, drm_hit_loci): locus 0 around the
// head row, then every further locus in the order the scan meets them, while its top still counts for the MAPQ
// (s >= sub_score - sub_band) or still passes as an alternative placement (s >= min_score and
// 100 * s >= drop_pct * best_score). Both tests are monotone in the non-increasing tops, so the scan stops at the first
// top that fails both, and the MAPQ record is hit_mapq_kernel's byte for byte.
//
// Mapping: one wave per read, the bounded grid of locus_scan.h looping with
// p += gridDim.x, the list staged in LDS by stage_list (12 bytes a row). max_loci <= 64, so lane j keeps slot j in four
// registers while the wave-uniform loop runs: recording a locus is one compare of the lane index against the uniform
// slot count and four selects, no store. After the loop the wave writes the read's max_loci slots of each of the four
// arrays in one coalesced pass (empty slots included, so every byte of the outputs is defined), lanes 0 to 7 write the
// eight words of the MAPQ record, and lane 0 the two counts.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "drm_device.h"
#include "locus_scan.h"

namespace drm {
namespace {

// 8 waves a SIMD: the bounded grid launches 32 one-wave blocks a CU for short lists, and with the 106 scalar registers
// the compiler takes unasked only 28 of them are resident, so the last four of every CU run as a second round
// (measured 1.38 x hit_mapq_kernel at k = 128 before this)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8))) void hit_loci_kernel(LociArgs a)
{
    extern __shared__ __align__(16) uint8_t smem[];
    const int cap = max(a.m.k, 1);
    uint64_t *lid = reinterpret_cast<uint64_t *>(smem);                  // [cap] window ids
    uint32_t *lst = reinterpret_cast<uint32_t *>(smem + 8 * (size_t)cap); // [cap] state words
    const int lane = threadIdx.x;
    const int k = a.m.k;
    const int max_loci = a.lp.max_loci;
    const drm_mapq_params &prm = a.m.prm;
    const uint64_t span_m1 = (uint64_t)(uint32_t)max(prm.locus_span - 1, 0);

    for (int64_t p = blockIdx.x; p < a.m.nreads; p += gridDim.x) {
        const int c = __builtin_amdgcn_readfirstlane(min(max(a.m.cnt[p], 0), k));
        int h = a.m.head ? __builtin_amdgcn_readfirstlane(a.m.head[p]) : -1;
        const int full = __builtin_amdgcn_readfirstlane(a.m.full[p]);
        __syncthreads(); // the previous read has read its LDS
        const uint32_t top = (uint32_t)__builtin_amdgcn_readfirstlane(
            (int)stage_list(a.m.ids + p * k, a.m.scores + p * k, c, lane, lid, lst));
        __syncthreads();

        // the lane's slot, empty until the scan records locus `lane`
        uint64_t slot_id = ~(uint64_t)0;
        int32_t slot_score = 0, slot_row = -1, slot_size = 0;
        int32_t rec[8] = {-1, 0, 0, -1, 0, 0, 0, 1}; // the "nothing" record, in drm_mapq_result's order
        int n_loci = 0, n_pass = 0;

        // the head rule of locus_scan; the keys are wave-uniform and kept in scalar registers, so that the loop below
        // branches on scalars
        if (h == -1)
            h = top ? 1023 - (int)(top & 1023u) : -1;
        const uint32_t hv = h >= 0 && h < c ? (uint32_t)__builtin_amdgcn_readfirstlane((int)lst[h]) : kRemoved;
        if (!(hv & kRemoved)) {
            const int best_score = (int)(hv & kScoreMask);
            const uint64_t hw = lid[h];
            int rows0 = 0;
            uint32_t next = (uint32_t)__builtin_amdgcn_readfirstlane(
                (int)remove_locus(lid, lst, c, lane, hw, span_m1, kRemoved, rows0));
            if (lane == 0) {
                slot_id = hw;
                slot_score = best_score;
                slot_row = h;
                slot_size = rows0;
            }
            n_loci = n_pass = 1;
            const int sub_score = (int)(next >> 10);
            const int sub_row = next ? 1023 - (int)(next & 1023u) : -1;
            int n_sub = 0;
            for (int it = 0; it < c && next != 0; ++it) { // each trip removes at least its own top
                const int s = (int)(next >> 10), t = 1023 - (int)(next & 1023u);
                const bool counts_sub = s >= sub_score - prm.sub_band;
                const bool passes = s >= prm.min_score && 100 * (int64_t)s >= (int64_t)a.lp.drop_pct * best_score;
                if (!counts_sub && !passes)
                    break;
                n_sub += counts_sub;
                const uint64_t tw = lid[t];
                int rows = 0;
                next = (uint32_t)__builtin_amdgcn_readfirstlane(
                    (int)remove_locus(lid, lst, c, lane, tw, span_m1, kRemoved, rows));
                if (passes) {
                    ++n_pass;
                    if (n_loci < max_loci) {
                        if (lane == n_loci) {
                            slot_id = tw;
                            slot_score = s;
                            slot_row = t;
                            slot_size = rows;
                        }
                        ++n_loci;
                    }
                }
            }
            rec[0] = h;
            rec[1] = best_score;
            rec[2] = rows0;
            rec[3] = sub_row;
            rec[4] = sub_score;
            rec[5] = n_sub;
            rec[6] = mapq_value(best_score, sub_score, n_sub, full, prm.min_score);
            rec[7] = 0;
        }

        if (lane < max_loci) {
            const int64_t at = p * max_loci + lane;
            a.loci_ids[at] = slot_id;
            a.loci_scores[at] = slot_score;
            a.loci_rows[at] = slot_row;
            a.loci_size[at] = slot_size;
        }
        if (lane < 8) { // the record's eight words, one per lane
            int32_t v = rec[0];
#pragma unroll
            for (int f = 1; f < 8; ++f)
                v = lane == f ? rec[f] : v;
            reinterpret_cast<int32_t *>(a.m.out + p)[lane] = v;
        }
        if (lane == 0) {
            a.n_loci[p] = n_loci;
            a.n_pass[p] = n_pass;
        }
    }
}

} // namespace

void launch_hit_loci(const LociArgs &a, hipStream_t stream)
{
    if (a.m.nreads <= 0)
        return;
    check_k(a.m.k, "locus list");
    if (a.lp.max_loci < 1 || a.lp.max_loci > kMaxLoci)
        throw Error(DRM_ERR_UNSUPPORTED, "max_loci = " + std::to_string(a.lp.max_loci) + " outside [1, 64]: a lane of "
                                         "the wave keeps one slot");
    const size_t lds = (size_t)12 * std::max(a.m.k, 1);
    hipLaunchKernelGGL(hit_loci_kernel, dim3(bounded_grid(a.m.nreads, lds)), dim3(64), lds, stream, a);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
