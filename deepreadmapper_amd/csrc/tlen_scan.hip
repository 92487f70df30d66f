// deepreadmapper_amd/csrc/tlen_scan.hip -- the template-length histogram of a batch of read pairs, for gfx950.
//
// The step that turns the two mates' reranked hit lists into "this pair's mates each map uniquely, in this orientation,
// this far apart" (include/drm_hip.h, drm_tlen_scan): the samples from which drm_tlen_estimate reads the library's
// template-length window.
//
// Mapping: hit_mapq_kernel's, twice per item. One wave per pair, a bounded grid looping over the
// pairs with the static p += gridDim.x. Mate 1's list is staged in LDS and scanned from its top hit (locus_scan.h); its
// MAPQ, its confidence and the id of its best row stay in scalars while mate 2's list is staged over it and scanned the
// same way, so the LDS is one list's, 12 B per row. The class and the template length are wave-uniform 64-bit integer
// arithmetic. Lane 0 then writes the sample and, for a pair of class 1 to 3, adds one to its bin with one vector atomic:
// the bin's index is formed only under cls in 1..3 and T <= max_scan, so no id or score can reach outside the
// histogram. Every loop runs to a clamped count; nothing waits on data.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "drm_device.h"
#include "locus_scan.h"

namespace drm {
namespace {

struct MateScan {
    uint64_t w;     // the id of the record's best row; 0 without one
    int mapq;       // 0 for status 1
    bool confident; // status 0 and mapq >= min_mapq
};

// the locus scan of the list staged in (lid, lst) from its top hit; every value is wave-uniform and in scalars
__device__ __forceinline__ MateScan scan_mate(const uint64_t *lid, uint32_t *lst, int c, int lane, uint32_t top,
                                              int full, const TlenArgs &a)
{
    const LocusScan s = locus_scan(lid, lst, c, lane, -1, top, a.prm);
    MateScan m{0, 0, false};
    if (s.status == 0) {
        const uint64_t w = lid[s.best];
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32));
        m.w = ((uint64_t)hi << 32) | lo;
        m.mapq = mapq_value(s.best_score, s.sub_score, s.n_sub, full, a.prm.min_score);
        m.confident = m.mapq >= a.tlen.min_mapq;
    }
    return m;
}

__global__ __launch_bounds__(64) void tlen_scan_kernel(TlenArgs a)
{
    extern __shared__ __align__(16) uint8_t smem[];
    const int cap = max(a.k, 1);
    uint64_t *lid = reinterpret_cast<uint64_t *>(smem);                  // [cap] window ids
    uint32_t *lst = reinterpret_cast<uint32_t *>(smem + 8 * (size_t)cap); // [cap] state words
    const int lane = threadIdx.x;
    const int k = a.k;
    const uint64_t ref_len = (uint64_t)(uint32_t)a.prm.ref_len;
    const uint64_t max_scan = (uint64_t)(uint32_t)a.tlen.max_scan;

    for (int64_t p = blockIdx.x; p < a.npairs; p += gridDim.x) {
        const int64_t row = p * a.row_step;
        const int c1 = __builtin_amdgcn_readfirstlane(min(max(a.cnt1[row], 0), k));
        const int c2 = __builtin_amdgcn_readfirstlane(min(max(a.cnt2[row], 0), k));
        const int full1 = __builtin_amdgcn_readfirstlane(a.full1[row]);
        const int full2 = __builtin_amdgcn_readfirstlane(a.full2[row]);

        __syncthreads(); // the previous pair has read its LDS
        const uint32_t top1 = stage_list(a.ids1 + row * k, a.scores1 + row * k, c1, lane, lid, lst);
        __syncthreads();
        const MateScan m1 = scan_mate(lid, lst, c1, lane, top1, full1, a);
        __syncthreads(); // mate 1's list has been read: mate 2's goes over it
        const uint32_t top2 = stage_list(a.ids2 + row * k, a.scores2 + row * k, c2, lane, lid, lst);
        __syncthreads();
        const MateScan m2 = scan_mate(lid, lst, c2, lane, top2, full2, a);

        // ---- class and template length, the same on every lane; positions are below 2^63, so T < 2^64
        int cls = 0;
        uint64_t T = 0;
        if (m1.confident && m2.confident) {
            const uint64_t p1 = m1.w >> 1, p2 = m2.w >> 1;
            if (((m1.w ^ m2.w) & 1u) == 0) {
                cls = 3;
                T = (p1 > p2 ? p1 - p2 : p2 - p1) + ref_len;
            } else {
                const uint64_t pf = (m1.w & 1u) ? p2 : p1, pr = (m1.w & 1u) ? p1 : p2;
                cls = pr >= pf ? 1 : 2;
                T = (pr >= pf ? pr - pf : pf - pr) + ref_len;
            }
            if (T > max_scan) {
                cls = 4;
                T = 0;
            }
        }
        if (lane == 0) {
            if (a.samples)
                a.samples[p] = drm_tlen_sample{cls, (int32_t)T, m1.mapq, m2.mapq};
            if (cls >= 1 && cls <= 3 && T <= max_scan)
                atomicAdd(a.hist + (uint64_t)(cls - 1) * (max_scan + 1) + T, 1u);
        }
    }
}

} // namespace

void launch_tlen_scan(const TlenArgs &a, hipStream_t stream)
{
    if (a.npairs <= 0)
        return;
    check_k(a.k, "template-length");
    const size_t lds = (size_t)12 * std::max(a.k, 1);
    hipLaunchKernelGGL(tlen_scan_kernel, dim3(bounded_grid(a.npairs, lds)), dim3(64), lds, stream, a);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
