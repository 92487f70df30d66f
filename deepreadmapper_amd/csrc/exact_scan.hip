// deepreadmapper_amd/csrc/exact_scan.hip -- exhaustive k-nearest-neighbour scans: the PQ-ADC
// distance of every code of a loaded IndexHNSWPQ, and the fp32 squared L2 distance of every row of a matrix, each with
// the bits the graph searches report (drm_search: pq_common.h; drm_flat_search: l2_items in hnsw_flat_search.hip), so
// that the k smallest under the total order (distance, id) are the ground truth for a recall figure. No graph, heap
// or visited set: a workgroup owns a tile of queries and one slice of the base rows, scores every row of the slice
// against every query of the tile, and keeps per (query, slice) the k smallest 64-bit keys ord32(dist) << 32 | id.
// A second kernel merges a query's slices. Keys are unique, so the result is a set that no tiling can change.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "drm_device.h"
#include "pq_common.h"

#pragma clang fp contract(off)

namespace drm {
namespace {

constexpr int kScanThreads = 256;          // 4 waves per workgroup
constexpr int kQT = 8;                     // queries per tile (PQ 8x8: 8 LUTs of 8 KB, two workgroups per CU)
constexpr int kPqRowsPerThread = 2;        // PQ 8x8: codes per lane per step
constexpr int kMaxK = 1024;                // the rerank's candidate cap (kMaxCands)
constexpr int kMaxCap = 2048;              // survivor buffer entries per (query, slice): >= k + rows per step
constexpr int kMaxSlices = 1024;
constexpr int64_t kWorkspaceBytes = 256ll << 20;
constexpr uint64_t kEmpty = ~0ull;         // no key equals it: ids are below 2^31

std::atomic<int64_t> g_slice_rows{0};      // drm_exact_set_slice_rows (0: the default split)

struct ScanArgs {
    SearchArgs sa;      // PQ: x, d, M, nbits, ksub, dsub, code_size, centroids, codes, x_aligned16 (n = queries)
    const float *base;  // fp32: [n_base][d]
    int64_t n_base;     // rows scanned (PQ: ntotal)
    int64_t slice_rows; // rows per slice, a multiple of 64
    int32_t slices;
    int32_t k, cap;     // cap: survivor buffer entries, a power of two >= k + rows per step
    uint64_t *ws;       // [n][slices][cap]: survivors while a slice runs, its k smallest keys (ascending) after
};

struct MergeArgs {
    const uint64_t *ws;
    int32_t slices, k, cap, kp; // kp: power of two >= k
    float *D;
    int64_t *I;
    const uint64_t *labels; // fp32 index: I receives labels[id] (padding 2^64-1)
};

// the lean search kernel's adc8 (hnsw_pq_fast.hip), restated here so that file compiles to what it did: byte M of c
// times 4 in one SDWA shift, the 8 LUT reads in flight before the first add, the adds in sub-quantizer order
template <int M> __device__ __forceinline__ uint32_t scan_bx4(uint32_t c)
{
    uint32_t r;
    if constexpr (M == 0)
        asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(c));
    else if constexpr (M == 1)
        asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(c));
    else if constexpr (M == 2)
        asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(c));
    else
        asm("v_lshlrev_b32_sdwa %0, 2, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t scan_adc8(const float *lut, uint2 c)
{
    const char *b = reinterpret_cast<const char *>(lut);
    float lv[8];
    lv[0] = *reinterpret_cast<const float *>(b + scan_bx4<0>(c.x));
    lv[1] = *reinterpret_cast<const float *>(b + scan_bx4<1>(c.x) + 1024);
    lv[2] = *reinterpret_cast<const float *>(b + scan_bx4<2>(c.x) + 2048);
    lv[3] = *reinterpret_cast<const float *>(b + scan_bx4<3>(c.x) + 3072);
    lv[4] = *reinterpret_cast<const float *>(b + scan_bx4<0>(c.y) + 4096);
    lv[5] = *reinterpret_cast<const float *>(b + scan_bx4<1>(c.y) + 5120);
    lv[6] = *reinterpret_cast<const float *>(b + scan_bx4<2>(c.y) + 6144);
    lv[7] = *reinterpret_cast<const float *>(b + scan_bx4<3>(c.y) + 7168);
    float r = lv[0]; // +0.0 + x == x for a LUT entry (never -0.0)
#pragma unroll
    for (int m = 1; m < 8; ++m)
        r = __fadd_rn(r, lv[m]);
    return ord32_nonneg(r);
}

// ---- selection: per query of the tile a threshold (its current k-th key, kEmpty until k survivors were sorted)
// and a count of the keys appended to its buffer in global memory since.

// one wave appends its lanes' passing keys: ballot, one LDS atomic for the wave, prefix count within it. The step's
// room (cap - cnt >= rows per step) was checked by the whole workgroup before the step.
__device__ __forceinline__ void sel_append(bool pass, uint64_t key, uint64_t *buf, int *cnt, int lane)
{
    const uint64_t m = __ballot(pass);
    if (m == 0)
        return;
    int at = 0;
    if (lane == 0)
        at = atomicAdd(cnt, (int)__popcll((unsigned long long)m));
    at = __builtin_amdgcn_readfirstlane(at);
    if (pass)
        buf[at + (int)__popcll((unsigned long long)(m & lanes_below(lane)))] = key;
}

// bitonic sort of s[0 .. n2) ascending (n2 a power of two >= 2) by the whole workgroup; ends on a barrier
__device__ void wg_sort(uint64_t *s, int n2)
{
    const int tid = (int)threadIdx.x;
    for (int size = 2; size <= n2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (n2 >> 1); i += kScanThreads) {
                const int lo = 2 * i - (i & (stride - 1));
                const int hi = lo + stride;
                const uint64_t x = s[lo], y = s[hi];
                if ((x > y) == ((lo & size) == 0)) {
                    s[lo] = y;
                    s[hi] = x;
                }
            }
            __syncthreads();
        }
}

// the whole workgroup cuts one query's buffer to its k smallest keys (ascending) and tightens the threshold. c, the
// count every thread read behind a barrier, is uniform. With `final` the list is padded with kEmpty up to k.
__device__ void sel_compact(uint64_t *buf, int c, int *cnt, uint64_t *thr, uint64_t *srt, int k, bool final)
{
    const int tid = (int)threadIdx.x;
    int n2 = 64;
    while (n2 < c)
        n2 <<= 1;
    for (int i = tid; i < n2; i += kScanThreads)
        srt[i] = i < c ? buf[i] : kEmpty;
    __syncthreads();
    wg_sort(srt, n2);
    const int keep = c < k ? c : k;
    for (int i = tid; i < keep; i += kScanThreads)
        buf[i] = srt[i];
    if (final)
        for (int i = keep + tid; i < k; i += kScanThreads)
            buf[i] = kEmpty;
    if (tid == 0) {
        *cnt = keep;
        if (c >= k)
            *thr = srt[k - 1];
    }
    __syncthreads();
}

// after a step: every thread reads the tile's counts behind one barrier and leaves through another, so that the next
// step's appends cannot move a count that a slower wave has yet to read: the decision to compact is uniform
template <int QT>
__device__ __forceinline__ void sel_step_end(uint64_t *ws_tile, int64_t q_stride, int *cnt, uint64_t *thr,
                                             uint64_t *srt, int k, int cap, int step_rows)
{
    __syncthreads();
    int c[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t)
        c[t] = cnt[t];
    __syncthreads();
#pragma unroll
    for (int t = 0; t < QT; ++t)
        if (c[t] + step_rows > cap)
            sel_compact(ws_tile + t * q_stride, c[t], &cnt[t], &thr[t], srt, k, false);
}

template <int QT>
__device__ __forceinline__ void sel_finish(uint64_t *ws_tile, int64_t q_stride, int *cnt, uint64_t *thr,
                                           uint64_t *srt, int k)
{
    __syncthreads();
    for (int t = 0; t < QT; ++t)
        sel_compact(ws_tile + t * q_stride, cnt[t], &cnt[t], &thr[t], srt, k, true);
}

// ---- PQ-ADC scan. FAST8 (PQ 8 x 8, 16-B aligned queries): QT LUTs of 8 KB in static LDS, each lane scores its
// 8-byte codes against all of them, so the code stream is read once per tile. Otherwise QT = 1 and the LUT
// (M * ksub floats <= 64 KB, dynamic LDS) is read through pq_distance_code<false>.
// grid: x = query tile, y = slice; queries past n in the last tile repeat query n - 1 into workspace rows of their
// own that the merge never reads.
template <int QT, bool FAST8>
__global__ __launch_bounds__(kScanThreads) void exact_pq_kernel(ScanArgs a)
{
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ __align__(16) float lut_static[FAST8 ? QT * 2048 : 4];
    __shared__ uint64_t srt_static[FAST8 ? 1 : kMaxCap];
    __shared__ uint64_t thr[QT];
    __shared__ int cnt[QT];
    float *lut = FAST8 ? lut_static : reinterpret_cast<float *>(dyn);
    uint64_t *srt = FAST8 ? reinterpret_cast<uint64_t *>(dyn) : srt_static;

    const int tid = (int)threadIdx.x, lane = lane_id(), wave = tid >> 6;
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    const int sl = (int)blockIdx.y;
    if (tid < QT) {
        thr[tid] = kEmpty;
        cnt[tid] = 0;
    }
    if (FAST8) {
        for (int t = wave; t < QT; t += kScanThreads / 64) {
            const int64_t q = q0 + t < a.sa.n ? q0 + t : a.sa.n - 1;
            build_lut_m8_ptr<1>(a.sa.x + q * a.sa.d, a.sa.centroids, lut + t * 2048, lane);
        }
    } else {
        build_lut(a.sa, q0, lut, lane); // every wave writes the same entries
    }
    __syncthreads();

    const int64_t q_stride = (int64_t)a.slices * a.cap;
    uint64_t *ws_tile = a.ws + (q0 * a.slices + sl) * (int64_t)a.cap;
    const int64_t r0 = (int64_t)sl * a.slice_rows;
    const int64_t r1 = r0 + a.slice_rows < a.n_base ? r0 + a.slice_rows : a.n_base;
    constexpr int RPT = FAST8 ? kPqRowsPerThread : 1;
    constexpr int kStep = kScanThreads * RPT;

    for (int64_t b = r0; b < r1; b += kStep) {
        int64_t row[RPT];
        uint2 c8[RPT];
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
            row[r] = b + r * kScanThreads + tid;
            c8[r] = make_uint2(0u, 0u);
            if (FAST8 && row[r] < r1)
                c8[r] = reinterpret_cast<const uint2 *>(a.sa.codes)[row[r]];
        }
        // every distance of the step first, with no branch between them, so that the LUT reads of all QT * RPT sums
        // are in flight together; then one ballot tells whether any lane of the wave has anything to append (after
        // the first few thousand rows of a slice, almost never)
        uint64_t key[QT][RPT];
        bool pass[QT][RPT];
        bool any = false;
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const uint64_t th = thr[t];
#pragma unroll
            for (int r = 0; r < RPT; ++r) {
                const bool valid = row[r] < r1;
                uint32_t dk;
                if (FAST8)
                    dk = scan_adc8(lut + t * 2048, c8[r]);
                else
                    dk = valid ? ord32(pq_distance_code<false>(a.sa, lut, (int32_t)row[r], c8[r])) : 0xFFFFFFFFu;
                key[t][r] = ((uint64_t)dk << 32) | (uint32_t)row[r];
                pass[t][r] = valid && key[t][r] < th;
                any |= pass[t][r];
            }
        }
        if (__ballot(any) != 0) {
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int r = 0; r < RPT; ++r)
                    sel_append(pass[t][r], key[t][r], ws_tile + t * q_stride, &cnt[t], lane);
        }
        sel_step_end<QT>(ws_tile, q_stride, cnt, thr, srt, a.k, a.cap, kStep);
    }
    sel_finish<QT>(ws_tile, q_stride, cnt, thr, srt, a.k);
}

// ---- fp32 scan: squared L2 in the flat search kernel's order (l2_items, hnswlib's L2SqrSIMD16ExtAVX): accumulator
// i sums fl(fl(x[j] - y[j])^2) over j = i, i + 8, ... in order, then ((a0 + a1) + a2) + ... + a7. A lane owns a row
// and reads it 16 dims (64 B) at a time; the tile's queries are read at wave-uniform addresses.
template <int QT> __global__ __launch_bounds__(kScanThreads) void exact_l2_kernel(ScanArgs a)
{
    extern __shared__ __align__(16) unsigned char dyn[];
    __shared__ uint64_t thr[QT];
    __shared__ int cnt[QT];
    uint64_t *srt = reinterpret_cast<uint64_t *>(dyn);

    const int tid = (int)threadIdx.x, lane = lane_id();
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    const int sl = (int)blockIdx.y;
    const int d = a.sa.d;
    if (tid < QT) {
        thr[tid] = kEmpty;
        cnt[tid] = 0;
    }
    __syncthreads();
    const float *__restrict__ xq[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t)
        xq[t] = a.sa.x + (q0 + t < a.sa.n ? q0 + t : a.sa.n - 1) * d;

    const int64_t q_stride = (int64_t)a.slices * a.cap;
    uint64_t *ws_tile = a.ws + (q0 * a.slices + sl) * (int64_t)a.cap;
    const int64_t r0 = (int64_t)sl * a.slice_rows;
    const int64_t r1 = r0 + a.slice_rows < a.n_base ? r0 + a.slice_rows : a.n_base;

    for (int64_t b = r0; b < r1; b += kScanThreads) {
        const int64_t row = b + tid;
        const bool valid = row < r1;
        float acc[QT][8];
#pragma unroll
        for (int t = 0; t < QT; ++t)
#pragma unroll
            for (int i = 0; i < 8; ++i)
                acc[t][i] = 0.0f;
        if (valid) {
            const float4 *__restrict__ y4 = reinterpret_cast<const float4 *>(a.base + row * d);
            for (int j = 0; j < d; j += 16) {
                float y[16];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float4 v = y4[(j >> 2) + i];
                    y[4 * i + 0] = v.x;
                    y[4 * i + 1] = v.y;
                    y[4 * i + 2] = v.z;
                    y[4 * i + 3] = v.w;
                }
#pragma unroll
                for (int t = 0; t < QT; ++t)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float df = __fsub_rn(xq[t][j + i], y[i]);
                        acc[t][i & 7] = __fadd_rn(acc[t][i & 7], __fmul_rn(df, df));
                    }
            }
        }
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            float r = acc[t][0];
#pragma unroll
            for (int i = 1; i < 8; ++i)
                r = __fadd_rn(r, acc[t][i]);
            const uint64_t key = ((uint64_t)ord32(r) << 32) | (uint32_t)row;
            sel_append(valid && key < thr[t], key, ws_tile + t * q_stride, &cnt[t], lane);
        }
        sel_step_end<QT>(ws_tile, q_stride, cnt, thr, srt, a.k, a.cap, kScanThreads);
    }
    sel_finish<QT>(ws_tile, q_stride, cnt, thr, srt, a.k);
}

// ---- merge: one workgroup per query folds its slices' ascending k-lists into the k smallest keys and writes them as
// drm_search does: D ascending, ties by id, I int64, missing slots (+inf, -1)
__global__ __launch_bounds__(kScanThreads) void exact_merge_kernel(MergeArgs a)
{
    extern __shared__ __align__(16) unsigned char dyn[];
    uint64_t *s = reinterpret_cast<uint64_t *>(dyn); // [2 * kp]
    const int tid = (int)threadIdx.x;
    const int64_t q = blockIdx.x;
    const uint64_t *lists = a.ws + q * a.slices * (int64_t)a.cap;
    for (int i = tid; i < a.kp; i += kScanThreads)
        s[i] = i < a.k ? lists[i] : kEmpty;
    __syncthreads();
    for (int sl = 1; sl < a.slices; ++sl) {
        const uint64_t *l = lists + (int64_t)sl * a.cap;
        for (int i = tid; i < a.kp; i += kScanThreads)
            s[a.kp + i] = i < a.k ? l[i] : kEmpty;
        __syncthreads();
        wg_sort(s, 2 * a.kp);
    }
    for (int i = tid; i < a.k; i += kScanThreads) {
        const uint64_t key = s[i];
        const bool none = key == kEmpty;
        const int64_t id = (int64_t)(uint32_t)key;
        a.D[q * a.k + i] = none ? __uint_as_float(0x7F800000u) : unord32((uint32_t)(key >> 32));
        if (a.labels)
            reinterpret_cast<uint64_t *>(a.I)[q * a.k + i] = none ? kEmpty : a.labels[id];
        else
            a.I[q * a.k + i] = none ? -1 : id;
    }
}

int pow2_at_least(int v)
{
    int p = 64;
    while (p < v)
        p <<= 1;
    return p;
}

void check_launch(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        throw Error(DRM_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
}

enum ScanKind { kScanPq8 = 0, kScanPqAny = 1, kScanL2 = 2 }; // the values of drm_debug_exact_plan's `kind`

// The whole plan of one scan of n queries over n_base rows at k: every number run_scan launches with.
//   qt, step         queries per tile and base rows per step of the kind's kernel
//   cap              survivor buffer entries per (query, slice): the power of two >= k + step
//   slice_rows, slices   the split of n_base rows: one round of resident workgroups over the whole grid (2 per CU
//                    for PQ 8 x 8, 4 otherwise: a second round repeats every tile's LUT build and start-up sorts;
//                    1,024 queries over 1M codes took 1.81 ms at 4 slices, one round, against 2.53 ms at 8 and
//                    2.34 ms at 2, profiles/r08/slices_c3.txt), slices of 16 Ki rows or more; or the rows
//                    drm_exact_set_slice_rows asked for, raised until at most kMaxSlices slices remain
//   chunk, chunks    queries per launch, a multiple of qt whose partial lists fit kWorkspaceBytes, and the launches
struct ScanPlan {
    int qt, step, cap;
    int64_t slice_rows;
    int slices;
    int64_t chunk, chunks;
};

ScanPlan scan_plan(ScanKind kind, int64_t n, int64_t n_base, int k)
{
    ScanPlan p{};
    p.qt = kind == kScanPqAny ? 1 : kQT;
    p.step = kind == kScanPq8 ? kScanThreads * kPqRowsPerThread : kScanThreads;
    p.cap = pow2_at_least(k + p.step);
    const int64_t tiles = (n + p.qt - 1) / p.qt;
    const int wg_per_cu = kind == kScanPq8 ? 2 : 4;
    int64_t rows = g_slice_rows.load();
    if (rows <= 0) {
        int dev = 0, cus = 256;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        int64_t want = ((int64_t)wg_per_cu * std::max(cus, 1) + tiles - 1) / tiles;
        want = std::max<int64_t>(1, std::min<int64_t>(want, n_base / 16384));
        rows = (n_base + want - 1) / want;
    }
    rows = std::max<int64_t>(rows, (n_base + kMaxSlices - 1) / kMaxSlices);
    rows = std::max<int64_t>(64, (rows + 63) / 64 * 64);
    p.slice_rows = rows;
    p.slices = (int)std::max<int64_t>(1, (n_base + rows - 1) / rows);
    const int64_t per_query = (int64_t)p.slices * p.cap * 8;
    int64_t chunk = std::max<int64_t>(1, kWorkspaceBytes / per_query) / p.qt * p.qt;
    p.chunk = std::min(std::max<int64_t>(chunk, p.qt), tiles * p.qt);
    p.chunks = (n + p.chunk - 1) / p.chunk;
    return p;
}

// One scan by its plan: queries in chunks whose partial lists fit kWorkspaceBytes, each chunk a scan launch and a
// merge launch on `stream`; synchronises the stream and frees the workspace before it returns. ms (may be null):
// device time of the launches (events on `stream`).
void run_scan(ScanKind kind, ScanArgs a, float *d_D, int64_t *d_I, const uint64_t *d_labels, hipStream_t stream,
              double *ms)
{
    const int64_t n = a.sa.n;
    const int d = a.sa.d;
    const float *x = a.sa.x;
    const ScanPlan p = scan_plan(kind, n, a.n_base, a.k);
    const int qt = p.qt;
    const int64_t chunk = p.chunk;
    a.cap = p.cap;
    a.slice_rows = p.slice_rows;
    a.slices = p.slices;
    uint64_t *ws = nullptr;
    DRM_HIP_CHECK(hipMalloc(&ws, (size_t)(chunk * p.slices * p.cap * 8)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    try {
        if (ms) {
            DRM_HIP_CHECK(hipEventCreate(&e0));
            DRM_HIP_CHECK(hipEventCreate(&e1));
            DRM_HIP_CHECK(hipEventRecord(e0, stream));
        }
        a.ws = ws;
        for (int64_t c = 0; c < p.chunks; ++c) {
            const int64_t q0 = c * chunk, nq = std::min(chunk, n - q0);
            a.sa.x = x + q0 * d;
            a.sa.n = nq;
            const dim3 grid((unsigned)((nq + qt - 1) / qt), (unsigned)a.slices);
            const size_t srt_bytes = (size_t)a.cap * 8;
            if (kind == kScanPq8)
                hipLaunchKernelGGL((exact_pq_kernel<kQT, true>), grid, dim3(kScanThreads), srt_bytes, stream, a);
            else if (kind == kScanPqAny)
                hipLaunchKernelGGL((exact_pq_kernel<1, false>), grid, dim3(kScanThreads),
                                   (size_t)a.sa.M * a.sa.ksub * sizeof(float), stream, a);
            else
                hipLaunchKernelGGL((exact_l2_kernel<kQT>), grid, dim3(kScanThreads), srt_bytes, stream, a);
            check_launch("exact scan kernel");
            MergeArgs m{ws, a.slices, a.k, a.cap, pow2_at_least(a.k), d_D + q0 * a.k, d_I + q0 * a.k, d_labels};
            hipLaunchKernelGGL(exact_merge_kernel, dim3((unsigned)nq), dim3(kScanThreads), (size_t)m.kp * 16, stream, m);
            check_launch("exact merge kernel");
        }
        if (ms)
            DRM_HIP_CHECK(hipEventRecord(e1, stream));
        DRM_HIP_CHECK(hipStreamSynchronize(stream));
        if (ms) {
            float t = 0.f;
            DRM_HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
            *ms = t;
        }
    } catch (...) {
        (void)hipStreamSynchronize(stream);
        (void)hipFree(ws);
        if (e0)
            (void)hipEventDestroy(e0);
        if (e1)
            (void)hipEventDestroy(e1);
        throw;
    }
    (void)hipFree(ws);
    if (e0)
        (void)hipEventDestroy(e0);
    if (e1)
        (void)hipEventDestroy(e1);
}

void check_nk(int64_t n, int k)
{
    if (n <= 0)
        throw Error(DRM_ERR_ARG, "Query data is empty");
    if (n >= (int64_t)1 << 31)
        throw Error(DRM_ERR_ARG, "more than 2^31-1 queries in one call");
    if (k < 1 || k > kMaxK)
        throw Error(DRM_ERR_UNSUPPORTED, "exact search: k must be in [1, " + std::to_string(kMaxK) + "], got " +
                                             std::to_string(k));
}

} // namespace

int exact_query_tile() { return kQT; }

void exact_plan(int kind, int64_t n, int64_t n_base, int k, int64_t out[7])
{
    if (kind < kScanPq8 || kind > kScanL2 || n_base < 0 || n_base >= (int64_t)1 << 31 || !out)
        throw Error(DRM_ERR_ARG, "drm_debug_exact_plan: kind in [0, 2], 0 <= n_base < 2^31, an output");
    check_nk(n, k);
    const ScanPlan p = scan_plan((ScanKind)kind, n, n_base, k);
    out[0] = p.qt;
    out[1] = p.step;
    out[2] = p.cap;
    out[3] = p.slice_rows;
    out[4] = p.slices;
    out[5] = p.chunk;
    out[6] = p.chunks;
}

int64_t exact_set_slice_rows(int64_t rows)
{
    if (rows < 0)
        throw Error(DRM_ERR_ARG, "drm_exact_set_slice_rows: rows must be >= 0");
    rows = (rows + 63) / 64 * 64;
    g_slice_rows.store(rows);
    return rows;
}

void launch_exact_pq(const DeviceIndex &ix, const float *d_x, int64_t n, int k, float *d_D, int64_t *d_I,
                     hipStream_t stream, double *ms)
{
    check_nk(n, k);
    if (!d_x || !d_D || !d_I)
        throw Error(DRM_ERR_ARG, "null argument");
    if (ix.ntotal >= (int64_t)1 << 31)
        throw Error(DRM_ERR_UNSUPPORTED, "exact search: 2^31 codes or more");
    if ((int64_t)ix.pq_M * ix.ksub * (int64_t)sizeof(float) > 65536)
        throw Error(DRM_ERR_UNSUPPORTED, "exact search: PQ lookup table larger than 64 KB");
    ScanArgs a{};
    a.sa.x = d_x;
    a.sa.n = n;
    a.sa.d = ix.d;
    a.sa.M = ix.pq_M;
    a.sa.nbits = ix.pq_nbits;
    a.sa.ksub = ix.ksub;
    a.sa.dsub = ix.dsub;
    a.sa.code_size = ix.code_size;
    a.sa.centroids = ix.centroids;
    a.sa.codes = ix.codes;
    a.sa.ntotal = ix.ntotal;
    a.sa.x_aligned16 = ((uintptr_t)d_x % 16) == 0;
    a.n_base = ix.ntotal;
    a.k = k;
    const bool fast8 = ix.pq_M == 8 && ix.pq_nbits == 8 && ix.code_size == 8 && ix.dsub == 16 && a.sa.x_aligned16;
    run_scan(fast8 ? kScanPq8 : kScanPqAny, a, d_D, d_I, nullptr, stream, ms);
}

void launch_exact_l2(const float *d_base, int64_t n_base, int d, const float *d_x, int64_t n, int k, float *d_D,
                     int64_t *d_I, const uint64_t *d_labels, hipStream_t stream, double *ms)
{
    check_nk(n, k);
    if (d <= 0 || d % 16 != 0)
        throw Error(DRM_ERR_UNSUPPORTED, "exact fp32 search needs d % 16 == 0 (hnswlib L2SqrSIMD16Ext)");
    if (n_base < 0 || !d_x || !d_D || !d_I || (n_base > 0 && !d_base))
        throw Error(DRM_ERR_ARG, "null or negative argument");
    if (n_base >= (int64_t)1 << 31)
        throw Error(DRM_ERR_UNSUPPORTED, "exact search: 2^31 rows or more");
    if ((uintptr_t)d_base % 16 != 0)
        throw Error(DRM_ERR_ARG, "exact fp32 search: the base matrix must be 16-byte aligned");
    ScanArgs a{};
    a.sa.x = d_x;
    a.sa.n = n;
    a.sa.d = d;
    a.base = d_base;
    a.n_base = n_base;
    a.k = k;
    run_scan(kScanL2, a, d_D, d_I, d_labels, stream, ms);
}

} // namespace drm
