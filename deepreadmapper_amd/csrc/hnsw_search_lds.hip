// deepreadmapper_amd/csrc/hnsw_search_lds.hip -- the HNSW-PQ search with its heaps in LDS, for any max(efSearch, k)
// up to 4096: launch_hnsw_search (hnsw_search.hip) picks it when the heaps pass the 512 register slots of
// hnsw_pq_search_kernel<8>, or when forced (DRM_SEARCH_LDS_KERNEL=1). Same semantics and results as that kernel, and
// the same pq_common.h for the distance, the greedy descent and the wave reductions. What differs: the query is staged
// in LDS for the LUT build, the candidate and result heaps are faiss's arrays of (f32 distance, i32 id) in LDS,
// replayed on lane 0 (pop_min and count_below stay wave-parallel), and the output is a bitonic sort in LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>

#include "drm_device.h"
#include "pq_common.h"

#pragma clang fp contract(off)

namespace drm {
namespace {

struct DI {
    float d;
    int32_t i;
};

// faiss::CMax<float, TI>::cmp2 on the distances themselves (pq_common.h's compares their ord32 images)
__device__ __forceinline__ bool cmp2(float v1, float v2, int32_t i1, int32_t i2)
{
    return (v1 > v2) || ((v1 == v2) && (i1 > i2));
}

// faiss heap_push<CMax<float,int32>>(k, ...) on a 0-based LDS array (1-based internally)
__device__ void heap_push(DI *h, int k, float val, int32_t id)
{
    int i = k;
    while (i > 1) {
        int f = i >> 1;
        DI pf = h[f - 1];
        if (!cmp2(val, pf.d, id, pf.i))
            break;
        h[i - 1] = pf;
        i = f;
    }
    h[i - 1] = DI{val, id};
}

// faiss heap_pop<CMax<float,int32>>(k, ...)
__device__ void heap_pop(DI *h, int k)
{
    DI last = h[k - 1];
    int i = 1;
    for (;;) {
        int i1 = i << 1, i2 = i1 + 1;
        if (i1 > k)
            break;
        DI c1 = h[i1 - 1];
        DI c2 = (i2 <= k) ? h[i2 - 1] : c1;
        if ((i2 == k + 1) || cmp2(c1.d, c2.d, c1.i, c2.i)) {
            if (cmp2(last.d, c1.d, last.i, c1.i))
                break;
            h[i - 1] = c1;
            i = i1;
        } else {
            if (cmp2(last.d, c2.d, last.i, c2.i))
                break;
            h[i - 1] = c2;
            i = i2;
        }
    }
    h[i - 1] = h[k - 1];
}

// faiss heap_replace_top<CMax<float,int64>>(k, ...) -- labels are storage ids (< 2^31)
__device__ void heap_replace_top(DI *h, int k, float val, int32_t id)
{
    int i = 1;
    for (;;) {
        int i1 = i << 1, i2 = i1 + 1;
        if (i1 > k)
            break;
        DI c1 = h[i1 - 1];
        DI c2 = (i2 <= k) ? h[i2 - 1] : c1;
        if ((i2 == k + 1) || cmp2(c1.d, c2.d, c1.i, c2.i)) {
            if (cmp2(val, c1.d, id, c1.i))
                break;
            h[i - 1] = c1;
            i = i1;
        } else {
            if (cmp2(val, c2.d, id, c2.i))
                break;
            h[i - 1] = c2;
            i = i2;
        }
    }
    h[i - 1] = DI{val, id};
}

template <bool FAST8>
__global__ __launch_bounds__(64) void hnsw_pq_search_lds_kernel(SearchArgs a)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int lane = lane_id();
    // LDS carve-up (all offsets 16-byte aligned by construction on the host)
    float *lut = reinterpret_cast<float *>(smem);
    float *qv = lut + a.M * a.ksub;
    DI *cand = reinterpret_cast<DI *>(qv + ((a.d + 3) & ~3));
    DI *res = cand + ((a.ef + 1) & ~1);
    DI *nb = res + a.kpad;                                // 64 entries
    uint64_t *keys = reinterpret_cast<uint64_t *>(res);  // sort image, aliases res
    uint32_t *vis = a.visited + (size_t)blockIdx.x * (size_t)a.vis_words;
    int32_t *clr = a.clear_list + (size_t)blockIdx.x * (size_t)a.clear_cap;

    int64_t taken = 0;
    for (;;) {
        const int64_t q = wave_next_item(a.counter, lane);
        if (q >= a.n)
            break;
        if (++taken > a.item_bound) { // more items than the queue holds: a broken work-queue fetch
            if (lane == 0)
                atomicAdd(a.errors, 1u);
            break;
        }

        // --- HeapBlockResultHandler::begin: heapify k x (+inf, -1)
        for (int j = lane; j < a.k; j += 64)
            res[j] = DI{INFINITY, -1};
        if (a.entry_point < 0 || a.ntotal == 0) {
            for (int j = lane; j < a.k; j += 64) {
                a.D[q * a.k + j] = INFINITY;
                a.I[q * a.k + j] = -1;
            }
            if (lane == 0) {
                a.ndis[q] = 0;
                a.nhops[q] = 0;
                if (a.nhops_upper)
                    a.nhops_upper[q] = 0;
            }
            continue;
        }
        // --- set_query: query vector to LDS, then LUT[m][c] = sum_t (x - c)^2 (sequential t)
        for (int t = lane; t < a.d; t += 64)
            qv[t] = a.x[q * a.d + t];
        __syncthreads();
        for (int e = lane; e < a.M * a.ksub; e += 64) {
            const int m = e / a.ksub;
            const float *cen = a.centroids + (size_t)e * a.dsub;
            const float *xs = qv + m * a.dsub;
            float acc = 0.0f;
            for (int t = 0; t < a.dsub; ++t) {
                float diff = __fsub_rn(xs[t], cen[t]);
                acc = __fadd_rn(acc, __fmul_rn(diff, diff));
            }
            lut[e] = acc;
        }
        __syncthreads();

        // --- greedy descent on levels max_level .. 1 (greedy_update_nearest)
        int32_t nearest;
        uint32_t dn;
        int ndis, nhops;
        greedy_upper<FAST8>(a, lut, lane, nearest, dn, ndis, nhops);
        const float d_nearest = unord32(dn); // the heaps hold the distance itself: ord32's exact inverse

        // --- level 0: MinimaxHeap candidates(ef); push(nearest); seed result + visited
        int kc = 1, nvalid = 1;
        if (lane == 0)
            cand[0] = DI{d_nearest, nearest};
        float thr = INFINITY;
        if (lane == 0) {
            if (d_nearest < thr) {
                heap_replace_top(res, a.k, d_nearest, nearest);
                thr = res[0].d;
            }
        }
        thr = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(thr)));
        int clear_n = 0;
        if (lane == 0) {
            atomicOr(&vis[nearest >> 5], 1u << (nearest & 31));
            if (a.clear_cap > 0)
                clr[0] = nearest;
        }
        clear_n = 1;
        __syncthreads();

        int nstep = 0, ndis0 = 0;
        bool overrun = false;
        while (nvalid > 0) {
            if (nstep > a.hop_bound) { // a node is expanded at most once: past the bound the bookkeeping is broken
                overrun = true;
                break;
            }
            // pop_min: min distance over valid slots, ties -> highest slot
            uint64_t best = ~0ull;
            for (int s = lane; s < kc; s += 64) {
                const DI e = cand[s];
                if (e.i != -1) {
                    uint64_t key = ((uint64_t)ord32(e.d) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)s);
                    best = key < best ? key : best;
                }
            }
            best = wave_min_u64_lanes(best); // not the wave-uniform form: 1.5 % slower here
            const int imin = (int)(0xFFFFFFFFu - (uint32_t)best);
            const DI pm = cand[imin];
            const float d0 = pm.d;
            const int32_t v0 = pm.i;
            __syncthreads();
            if (lane == 0)
                cand[imin].i = -1;
            nvalid--;
            // count_below(d0): every slot < kc, popped ones included
            int below = 0;
            for (int base = 0; base < kc; base += 64) {
                const int s = base + lane;
                const bool b = (s < kc) && (cand[s].d < d0);
                below += __popcll(__ballot(b));
            }
            if (below >= a.efSearch)
                break;

            // expand v0's level-0 row
            const int32_t *row = a.nbr0 + (size_t)v0 * (size_t)a.deg0;
            const int32_t v1 = (lane < a.deg0) ? row[lane] : -1;
            const uint64_t negm = __ballot(lane < a.deg0 && v1 < 0);
            const int jmax = negm ? (__ffsll((unsigned long long)negm) - 1) : a.deg0;
            bool fresh = false;
            if (lane < jmax) {
                const uint32_t bit = 1u << (v1 & 31);
                const uint32_t old = atomicOr(&vis[v1 >> 5], bit);
                fresh = (old & bit) == 0u;
            }
            if (a.check_dups) { // a repeated id in one row: only its first occurrence is fresh
                for (int j = 0; j < jmax; ++j) {
                    const int32_t vj = __shfl(v1, j, 64);
                    if (j < lane && vj == v1)
                        fresh = false;
                }
            }
            const uint64_t fm = __ballot(fresh);
            const int nf = __popcll(fm);
            const int pos = __popcll(fm & lanes_below(lane));
            if (fresh) {
                if (clear_n + pos < a.clear_cap)
                    clr[clear_n + pos] = v1;
                const float dd = pq_distance_code<FAST8>(a, lut, v1, load_code8<FAST8>(a, v1));
                nb[pos] = DI{dd, v1};
            }
            clear_n += nf;
            ndis0 += nf;
            __syncthreads();
            if (lane == 0) {
                // add_to_heap for each fresh link, in row order
                for (int t = 0; t < nf; ++t) {
                    const DI e = nb[t];
                    if (e.d < thr) {
                        heap_replace_top(res, a.k, e.d, e.i);
                        thr = res[0].d;
                    }
                    // MinimaxHeap::push
                    if (kc == a.ef) {
                        const DI top = cand[0];
                        if (e.d >= top.d)
                            continue;
                        if (top.i != -1)
                            --nvalid;
                        heap_pop(cand, kc--);
                    }
                    heap_push(cand, ++kc, e.d, e.i);
                    ++nvalid;
                }
            }
            kc = __builtin_amdgcn_readfirstlane(kc);
            nvalid = __builtin_amdgcn_readfirstlane(nvalid);
            thr = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(thr)));
            __syncthreads();
            nstep++;
        }

        // --- SingleResultHandler::end (heap_reorder): ascending (distance, id), (+inf,-1) padding
        __syncthreads();
        for (int j = lane; j < a.kpad; j += 64) { // in place: keys[j] aliases res[j] (both 8 bytes)
            const DI e = (j < a.k) ? res[j] : DI{INFINITY, -1};
            keys[j] = (e.i >= 0) ? (((uint64_t)ord32(e.d) << 32) | (uint32_t)e.i) : ~0ull;
        }
        __syncthreads();
        for (int size = 2; size <= a.kpad; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = lane; t < (a.kpad >> 1); t += 64) {
                    const int i = 2 * t - (t & (stride - 1));
                    const int j = i + stride;
                    const bool asc = (i & size) == 0;
                    const uint64_t x = keys[i], y = keys[j];
                    if ((x > y) == asc) {
                        keys[i] = y;
                        keys[j] = x;
                    }
                }
                __syncthreads();
            }
        }
        for (int j = lane; j < a.k; j += 64) {
            const uint64_t key = keys[j];
            if (key == ~0ull) {
                a.D[q * a.k + j] = INFINITY;
                a.I[q * a.k + j] = -1;
            } else {
                a.D[q * a.k + j] = unord32((uint32_t)(key >> 32));
                a.I[q * a.k + j] = (int64_t)(uint32_t)key;
            }
        }
        if (lane == 0) {
            a.ndis[q] = overrun ? -1 : ndis + ndis0;
            a.nhops[q] = overrun ? -1 : nhops + nstep;
            if (a.nhops_upper)
                a.nhops_upper[q] = nhops;
            if (overrun)
                atomicAdd(a.errors, 1u);
        }

        // --- VisitedTable::advance: clear exactly the bits this query set
        if (clear_n <= a.clear_cap) {
            for (int t = lane; t < clear_n; t += 64)
                vis[clr[t] >> 5] = 0u;
        } else {
            for (int64_t w = lane; w < a.vis_words; w += 64)
                vis[w] = 0u;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

} // namespace

void launch_hnsw_pq_lds(const SearchArgs &a, int slots, size_t lds_bytes, bool fast8, hipStream_t stream)
{
    if (fast8)
        hipLaunchKernelGGL(hnsw_pq_search_lds_kernel<true>, dim3(slots), dim3(64), lds_bytes, stream, a);
    else
        hipLaunchKernelGGL(hnsw_pq_search_lds_kernel<false>, dim3(slots), dim3(64), lds_bytes, stream, a);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
