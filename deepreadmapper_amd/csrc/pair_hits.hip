// deepreadmapper_amd/csrc/pair_hits.hip -- mate pairing of two reads' reranked hit lists, for gfx950.
//
// The step between the SW rerank and the alignment of a read pair (include/drm_hip.h, drm_pair_hits): of the up to
// k x k combinations of a hit of mate 1 with a hit of mate 2, count the proper ones (opposite strands, forward hit
// left of the reverse hit, template length inside [min_tlen, max_tlen]) and choose the best by (score sum, row of
// mate 1, row of mate 2); fall back to the mates' top hits when no proper combination comes within unpaired_penalty
// of them.
//
// Mapping: one wave per pair, a bounded grid looping over pairs. Mate 2's live rows are staged in
// LDS split by strand -- forward rows packed from the front of the arrays, reverse rows from the back (a ballot and a
// popcount per 64 rows give each row its slot) -- as (position u64, score << 10 | 1023 - j2), 12 bytes per row, 12 KB at
// k = 1024: a row of mate 1 then meets only the rows of the other strand, and the word already holds the row's share of
// the key. Mate 1's rows are loaded 64 at a time, one per lane, and walked wave-uniformly through v_readlane; inside,
// lanes stride over the sublist. The template-length test is one unsigned 64-bit range check,
// (pos2 - pos1 - dlo) <= dhi - dlo for a forward row of mate 1 and (pos1 - dlo - pos2) <= dhi - dlo for a reverse
// one, dlo = max(0, min_tlen - ref_len), dhi = max_tlen - ref_len: positions are below 2^63, so the difference never
// aliases into the range. Every lane keeps one 64-bit key, sum << 32 | (1023 - j1) << 10 | (1023 - j2), whose maximum
// is the choice and its tie rule at once, reduced by one butterfly per pair; the proper rows are counted by ballot. The top hits are the
// maxima of score << 10 | (1023 - j) over each list. Every loop runs to a count clamped to [0, k].
#include <hip/hip_runtime.h>

#include <algorithm>

#include "drm_device.h"

namespace drm {
namespace {

__device__ __forceinline__ uint64_t readlane64(uint64_t x, int l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t umax64(uint64_t x, uint64_t y) { return x > y ? x : y; }

__device__ __forceinline__ uint64_t wave_max64(uint64_t x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, off);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), off);
        x = umax64(x, ((uint64_t)hi << 32) | lo);
    }
    return x;
}

__device__ __forceinline__ uint32_t wave_max32(uint32_t x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        x = max(x, (uint32_t)__shfl_xor((int)x, off));
    return x;
}

// the lane's share of rows [begin, end) of one strand of mate 2 against one row of mate 1 of the other strand. REV1:
// that row is the reverse hit, so a (forward) row at pos2 <= pos1 pairs with it; otherwise a (reverse) row at
// pos2 >= pos1. `edge` is pos1 + dlo (forward) or pos1 - dlo (reverse), `key1` the row's part of the key.
template <bool REV1>
__device__ __forceinline__ void pair_row(const uint64_t *lpos, const uint32_t *lsw, int begin, int end, int lane,
                                         uint64_t edge, uint64_t range, uint32_t s1, uint32_t key1, uint64_t &best,
                                         int &n)
{
    for (int i = begin + lane; i < end; i += 64) {
        const uint32_t sw = lsw[i];
        const uint64_t pos2 = lpos[i];
        const uint64_t x = REV1 ? edge - pos2 : pos2 - edge;
        const bool proper = x <= range;
        const uint64_t key = ((uint64_t)(s1 + (sw >> 10)) << 32) | key1 | (sw & 1023u);
        best = (proper & (key > best)) ? key : best;
        n += __popcll(__ballot(proper)); // the active lanes' proper rows, counted on the scalar unit
    }
}

__global__ __launch_bounds__(64) void pair_hits_kernel(PairArgs a)
{
    extern __shared__ __align__(16) uint8_t smem[];
    const int cap = max(a.k, 1);
    uint64_t *lpos = reinterpret_cast<uint64_t *>(smem);                      // [cap] positions of mate 2's live rows:
    uint32_t *lsw = reinterpret_cast<uint32_t *>(smem + 8 * (size_t)cap);     // [cap] score << 10 | (1023 - j2);
    // forward rows in [0, nf), reverse rows in [cap - nr, cap)
    const int lane = threadIdx.x;
    const int k = a.k;
    const int64_t dlo = max(a.prm.min_tlen - a.prm.ref_len, 0);
    const int64_t dhi = (int64_t)a.prm.max_tlen - a.prm.ref_len;
    const bool any_range = dhi >= dlo; // otherwise no template length is accepted
    const uint64_t range = (uint64_t)(dhi - dlo);

    for (int64_t p = blockIdx.x; p < a.npairs; p += gridDim.x) {
        const int64_t row = p * a.row_step;
        const int c1 = __builtin_amdgcn_readfirstlane(min(max(a.cnt1[row], 0), k));
        const int c2 = __builtin_amdgcn_readfirstlane(min(max(a.cnt2[row], 0), k));
        const uint64_t *i1 = a.ids1 + row * k, *i2 = a.ids2 + row * k;
        const int32_t *sc1 = a.scores1 + row * k, *sc2 = a.scores2 + row * k;

        __syncthreads(); // the previous pair has read its LDS
        uint32_t top2 = 0;
        int nf = 0, nr = 0;
        for (int base = 0; base < c2; base += 64) {
            const int j = base + lane;
            const uint64_t w = j < c2 ? i2[j] : 0;
            const int sc = j < c2 ? sc2[j] : 0;
            const bool live = sc > 0, rev = (w & 1u) != 0;
            const uint32_t sw = ((uint32_t)sc << 10) | (uint32_t)(1023 - j);
            const uint64_t mf = __ballot(live && !rev), mr = __ballot(live && rev);
            const uint64_t below = ((uint64_t)1 << lane) - 1;
            if (live) {
                const int at = rev ? cap - 1 - (nr + __popcll(mr & below)) : nf + __popcll(mf & below);
                lpos[at] = w >> 1;
                lsw[at] = sw;
                top2 = max(top2, sw);
            }
            nf += __popcll(mf);
            nr += __popcll(mr);
        }
        __syncthreads();

        uint64_t best = 0;
        uint32_t top1 = 0;
        int n = 0;
        for (int base = 0; base < c1; base += 64) {
            const int j = base + lane;
            const uint64_t w1 = j < c1 ? i1[j] : 0;
            const int s1 = j < c1 ? sc1[j] : 0;
            if (s1 > 0)
                top1 = max(top1, ((uint32_t)s1 << 10) | (uint32_t)(1023 - j));
            const int lim = any_range ? min(64, c1 - base) : 0;
            for (int t = 0; t < lim; ++t) {
                const int s1u = __builtin_amdgcn_readlane(s1, t);
                if (s1u <= 0)
                    continue;
                const uint64_t w1u = readlane64(w1, t);
                const uint64_t pos1 = w1u >> 1;
                const uint32_t key1 = (uint32_t)(1023 - (base + t)) << 10;
                if (w1u & 1u)
                    pair_row<true>(lpos, lsw, 0, nf, lane, pos1 - (uint64_t)dlo, range, (uint32_t)s1u, key1, best, n);
                else
                    pair_row<false>(lpos, lsw, cap - nr, cap, lane, pos1 + (uint64_t)dlo, range, (uint32_t)s1u, key1,
                                    best, n);
            }
        }
        best = wave_max64(best);
        // lane 0 takes every trip of pair_row's loop that any lane takes, so its count saw every ballot
        n = __builtin_amdgcn_readfirstlane(n);
        top1 = wave_max32(top1);
        top2 = wave_max32(top2);

        // ---- the record, the same on every lane
        const int t1 = top1 ? 1023 - (int)(top1 & 1023u) : -1, t2 = top2 ? 1023 - (int)(top2 & 1023u) : -1;
        const int st1 = (int)(top1 >> 10), st2 = (int)(top2 >> 10);
        drm_pair_result r;
        r.n_proper = n;
        r.tlen = 0;
        if (top1 && top2) {
            const int best_sum = (int)(best >> 32);
            if (n > 0 && best_sum >= st1 + st2 - a.prm.unpaired_penalty) {
                r.j1 = 1023 - (int)((best >> 10) & 1023u);
                r.j2 = 1023 - (int)(best & 1023u);
                r.score = best_sum;
                const uint64_t wa = i1[r.j1], pa = wa >> 1, pb = i2[r.j2] >> 1;
                const uint64_t pf = (wa & 1u) ? pb : pa, pr = (wa & 1u) ? pa : pb;
                r.tlen = (int32_t)(pr - pf + (uint64_t)a.prm.ref_len);
                r.status = 0;
            } else {
                r.j1 = t1;
                r.j2 = t2;
                r.score = st1 + st2;
                r.status = 1;
            }
        } else {
            r.j1 = t1;
            r.j2 = t2;
            r.score = st1 + st2; // the live mate's top score, or 0
            r.status = top1 ? 2 : top2 ? 3 : 4;
        }
        if (lane == 0)
            a.out[p] = r;
    }
}

} // namespace

void launch_pair_hits(const PairArgs &a, hipStream_t stream)
{
    if (a.npairs <= 0)
        return;
    if (a.k < 0 || a.k > kMaxCands)
        throw Error(DRM_ERR_UNSUPPORTED, "k = " + std::to_string(a.k) + " outside [0, 1024]: the pairing kernel keeps "
                                         "one list of the rerank's candidate cap in LDS");
    int dev = 0, cus = 0;
    DRM_HIP_CHECK(hipGetDevice(&dev));
    DRM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // bounded grid, each wave loops over pairs: as many waves per CU as its 160 KB of LDS hold, 32 at the most (8 per
    // SIMD; the kernel waits on LDS and v_readlane chains at small k, which more waves hide), a multiple of the 4 SIMDs
    const size_t lds = (size_t)12 * std::max(a.k, 1);
    const int per_cu = std::max((int)std::min<size_t>(32, (size_t)160 * 1024 / lds) & ~3, 4);
    const int grid = (int)std::min<int64_t>(a.npairs, (int64_t)std::max(cus, 1) * per_cu);
    hipLaunchKernelGGL(pair_hits_kernel, dim3(grid), dim3(64), lds, stream, a);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
