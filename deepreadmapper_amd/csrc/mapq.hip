// deepreadmapper_amd/csrc/mapq.hip -- mapping quality from a read's reranked hit list, for gfx950.
//
// The step that turns "k window ids with their scores" into "best locus, best competing locus, how many competitors"
// (include/drm_hip.h, drm_hit_mapq), and for a read pair the best proper combination that is not the chosen one
// shifted by a few bases (drm_pair_mapq). At stride 1 the windows beside the true one overlap it and score almost as
// high, so the list is collapsed into loci first: a greedy non-maximum suppression over positions.
//
// Mapping: one wave per read / per pair, a bounded grid looping over the items with the static
// p += gridDim.x. The staging of a list in LDS and the scan over it are locus_scan.h's, which tlen_scan.hip shares.
// The pair kernel scans mate 2's list with head j2, packs its live rows split by strand as pair_hits_kernel does --
// (position, score | in-locus-0 << 31) -- then scans mate 1's list in the same staging arrays with head j1 and walks
// its rows wave-uniformly over the other strand's sublist: a row of mate 1 inside the chosen locus masks out the rows of
// mate 2 inside theirs, so the excluded combinations drop out of the maximum.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "drm_device.h"
#include "locus_scan.h"

namespace drm {
namespace {

__device__ __forceinline__ uint64_t readlane64(uint64_t x, int l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(64) void hit_mapq_kernel(MapqArgs a)
{
    extern __shared__ __align__(16) uint8_t smem[];
    const int cap = max(a.k, 1);
    uint64_t *lid = reinterpret_cast<uint64_t *>(smem);                  // [cap] window ids
    uint32_t *lst = reinterpret_cast<uint32_t *>(smem + 8 * (size_t)cap); // [cap] state words
    const int lane = threadIdx.x;
    const int k = a.k;

    for (int64_t p = blockIdx.x; p < a.nreads; p += gridDim.x) {
        const int c = __builtin_amdgcn_readfirstlane(min(max(a.cnt[p], 0), k));
        const int head = a.head ? __builtin_amdgcn_readfirstlane(a.head[p]) : -1;
        const int full = __builtin_amdgcn_readfirstlane(a.full[p]);
        __syncthreads(); // the previous read has read its LDS
        const uint32_t top = stage_list(a.ids + p * k, a.scores + p * k, c, lane, lid, lst);
        __syncthreads();
        const LocusScan s = locus_scan(lid, lst, c, lane, head, top, a.prm);
        drm_mapq_result r;
        r.best = s.best;
        r.best_score = s.best_score;
        r.locus_rows = s.locus_rows;
        r.sub_row = s.sub_row;
        r.sub_score = s.sub_score;
        r.n_sub = s.n_sub;
        r.mapq = s.status == 0 ? mapq_value(s.best_score, s.sub_score, s.n_sub, full, a.prm.min_score) : 0;
        r.status = s.status;
        if (lane == 0)
            a.out[p] = r;
    }
}

// the lane's share of rows [begin, end) of one strand of mate 2 against one row of mate 1 of the other strand
// (pair_hits_kernel's pair_row, keeping only the largest sum): a row whose word has a bit of `mask` is excluded
template <bool REV1>
__device__ __forceinline__ void sub_pair_row(const uint64_t *lpos, const uint32_t *lsw, int begin, int end, int lane,
                                             uint64_t edge, uint64_t range, uint32_t s1, uint32_t mask, uint32_t &best)
{
    for (int i = begin + lane; i < end; i += 64) {
        const uint32_t sw = lsw[i];
        const uint64_t pos2 = lpos[i];
        const uint64_t x = REV1 ? edge - pos2 : pos2 - edge;
        const bool ok = x <= range && !(sw & mask);
        const uint32_t sum = s1 + (sw & kScoreMask);
        best = (ok && sum > best) ? sum : best;
    }
}

__global__ __launch_bounds__(64) void pair_mapq_kernel(PairMapqArgs a)
{
    extern __shared__ __align__(16) uint8_t smem[];
    const int k = a.pair.k;
    const int cap = (max(k, 1) + 1) & ~1; // even: the u64 arrays stay 8-byte aligned
    uint64_t *lid = reinterpret_cast<uint64_t *>(smem);                       // [cap] the list being scanned
    uint64_t *lpos = reinterpret_cast<uint64_t *>(smem + 8 * (size_t)cap);    // [cap] positions of mate 2's live rows:
    uint32_t *lst = reinterpret_cast<uint32_t *>(smem + 16 * (size_t)cap);    // [cap] state words of the scanned list
    uint32_t *lsw = reinterpret_cast<uint32_t *>(smem + 20 * (size_t)cap);    // [cap] score | in locus 0 << 31;
    // forward rows in [0, nf), reverse rows in [cap - nr, cap)
    const int lane = threadIdx.x;
    const drm_pair_params &pp = a.pair.prm;
    const int64_t dlo = max(pp.min_tlen - pp.ref_len, 0);
    const int64_t dhi = (int64_t)pp.max_tlen - pp.ref_len;
    const bool any_range = dhi >= dlo;
    const uint64_t range = (uint64_t)(dhi - dlo);

    for (int64_t p = blockIdx.x; p < a.pair.npairs; p += gridDim.x) {
        const int64_t row = p * a.pair.row_step;
        const int c1 = __builtin_amdgcn_readfirstlane(min(max(a.pair.cnt1[row], 0), k));
        const int c2 = __builtin_amdgcn_readfirstlane(min(max(a.pair.cnt2[row], 0), k));
        const int full1 = __builtin_amdgcn_readfirstlane(a.full1[row]);
        const int full2 = __builtin_amdgcn_readfirstlane(a.full2[row]);
        const int j1 = __builtin_amdgcn_readfirstlane(a.pairs[p].j1);
        const int j2 = __builtin_amdgcn_readfirstlane(a.pairs[p].j2);
        const int score = __builtin_amdgcn_readfirstlane(a.pairs[p].score);
        const int status = __builtin_amdgcn_readfirstlane(a.pairs[p].status);
        const bool known = status >= 0 && status <= 3; // status 4, or a record outside the contract: all zero
        const bool table = status == 0 && any_range;

        // ---- mate 2: its scan with head j2, then its live rows split by strand with the locus bit
        __syncthreads(); // the previous pair has read its LDS
        const uint32_t top2 = stage_list(a.pair.ids2 + row * k, a.pair.scores2 + row * k, c2, lane, lid, lst);
        __syncthreads();
        LocusScan s2{-1, 0, 0, -1, 0, 0, 1};
        if (known && j2 >= 0)
            s2 = locus_scan(lid, lst, c2, lane, j2, top2, a.prm);
        int nf = 0, nr = 0;
        if (table) {
            for (int base = 0; base < c2; base += 64) {
                const int j = base + lane;
                const uint32_t v = j < c2 ? lst[j] : 0u; // the lane's own rows
                const uint64_t w = j < c2 ? lid[j] : 0;
                const uint32_t sc = v & kScoreMask;
                const bool live = sc != 0, rev = (w & 1u) != 0;
                const uint64_t mf = __ballot(live && !rev), mr = __ballot(live && rev);
                const uint64_t below = ((uint64_t)1 << lane) - 1;
                if (live) {
                    const int at = rev ? cap - 1 - (nr + __popcll(mr & below)) : nf + __popcll(mf & below);
                    lpos[at] = w >> 1;
                    lsw[at] = sc | ((v & kLocus0) ? kRemoved : 0u);
                }
                nf += __popcll(mf);
                nr += __popcll(mr);
            }
        }

        // ---- mate 1: its scan with head j1 in the same staging arrays
        __syncthreads();
        const uint32_t top1 = stage_list(a.pair.ids1 + row * k, a.pair.scores1 + row * k, c1, lane, lid, lst);
        __syncthreads();
        LocusScan s1{-1, 0, 0, -1, 0, 0, 1};
        if (known && j1 >= 0)
            s1 = locus_scan(lid, lst, c1, lane, j1, top1, a.prm);

        // ---- the best proper combination outside (locus 0 of mate 1) x (locus 0 of mate 2)
        uint32_t sub_pair = 0;
        if (table) {
            for (int base = 0; base < c1; base += 64) {
                const int j = base + lane;
                const uint32_t v1 = j < c1 ? lst[j] : 0u;
                const uint64_t w1 = j < c1 ? lid[j] : 0;
                const int lim = min(64, c1 - base);
                for (int t = 0; t < lim; ++t) {
                    const uint32_t vu = (uint32_t)__builtin_amdgcn_readlane((int)v1, t);
                    const uint32_t s1u = vu & kScoreMask;
                    if (s1u == 0)
                        continue;
                    const uint64_t w1u = readlane64(w1, t);
                    const uint64_t pos1 = w1u >> 1;
                    const uint32_t mask = (vu & kLocus0) ? kRemoved : 0u;
                    if (w1u & 1u)
                        sub_pair_row<true>(lpos, lsw, 0, nf, lane, pos1 - (uint64_t)dlo, range, s1u, mask, sub_pair);
                    else
                        sub_pair_row<false>(lpos, lsw, cap - nr, cap, lane, pos1 + (uint64_t)dlo, range, s1u, mask,
                                            sub_pair);
                }
            }
            sub_pair = wave_max32(sub_pair);
        }

        // ---- the record, the same on every lane
        drm_pair_mapq_result r{0, 0, 0, 0, 0, 0};
        if (known) {
            r.q_se1 = s1.status == 0 ? mapq_value(s1.best_score, s1.sub_score, s1.n_sub, full1, a.prm.min_score) : 0;
            r.q_se2 = s2.status == 0 ? mapq_value(s2.best_score, s2.sub_score, s2.n_sub, full2, a.prm.min_score) : 0;
            r.mapq1 = r.q_se1;
            r.mapq2 = r.q_se2;
            if (status == 0) {
                const int64_t unpaired = (int64_t)(top1 >> 10) + (int64_t)(top2 >> 10) - pp.unpaired_penalty;
                const int64_t subo = max((int64_t)sub_pair, unpaired);
                const int64_t q = 6 * ((int64_t)score - subo);
                r.sub_pair = (int32_t)sub_pair;
                r.q_pe = (int32_t)min(max(q, (int64_t)0), (int64_t)60);
                r.mapq1 = r.q_se1 > r.q_pe ? r.q_se1 : min(r.q_pe, r.q_se1 + 40);
                r.mapq2 = r.q_se2 > r.q_pe ? r.q_se2 : min(r.q_pe, r.q_se2 + 40);
            }
        }
        if (lane == 0)
            a.out[p] = r;
    }
}

} // namespace

void launch_hit_mapq(const MapqArgs &a, hipStream_t stream)
{
    if (a.nreads <= 0)
        return;
    check_k(a.k, "MAPQ");
    const size_t lds = (size_t)12 * std::max(a.k, 1);
    hipLaunchKernelGGL(hit_mapq_kernel, dim3(bounded_grid(a.nreads, lds)), dim3(64), lds, stream, a);
    DRM_HIP_CHECK(hipGetLastError());
}

void launch_pair_mapq(const PairMapqArgs &a, hipStream_t stream)
{
    if (a.pair.npairs <= 0)
        return;
    check_k(a.pair.k, "pair MAPQ");
    const size_t lds = (size_t)24 * ((std::max(a.pair.k, 1) + 1) & ~1);
    hipLaunchKernelGGL(pair_mapq_kernel, dim3(bounded_grid(a.pair.npairs, lds)), dim3(64), lds, stream, a);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
