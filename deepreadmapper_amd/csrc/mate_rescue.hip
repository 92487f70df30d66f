// deepreadmapper_amd/csrc/mate_rescue.hip -- mate rescue: the score-only affine-gap scan of a read over the insert
// window of its mate's hit, for gfx950.
//
// The step after drm_pair_hits for a pair that has no proper combination (include/drm_hip.h, drm_mate_rescue): the
// mate that mapped is the anchor, and the other read is aligned against the up to 2,048 genome bases in which the
// template length says it must lie. The recurrence and the end-cell rule are drm_sw_align_affine's; nothing is traced
// back, so no direction is stored, which is what lets the region be eight times the aligners' 256 rows.
//
// Mapping: that of sw_align_affine.hip -- one wave per task, lane l owns the C = LQ / 64 query
// columns [l * C, l * C + C), rows skewed by lane, H and E handed to the right neighbour in one DPP shift each per
// step, n + ceil(m / C) - 1 steps -- with plain values in place of the times-4 values whose low bits fed the walk.
// LDS holds the oriented region (staged once, complemented while staging) and the query: 2,304 bytes per wave.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sw_wave.h"

namespace drm {
namespace {

constexpr int kNegInf = -(1 << 20); // the borders' E and F: below every real value, far from overflow

// the best cell's key (sw_wave.h): H <= 31 * 256 < 2^13, rows are 0-based and below 2^11
using RescueKey = CellKey<19, 0>;
static_assert(kRescueMaxRows == RescueKey::kRowMax + 1, "11 bits of row");
static_assert(31 * kAlignMaxLen < 1 << (32 - RescueKey::kHShift), "13 bits of score");

template <int LQ>
__global__ __launch_bounds__(64) void mate_rescue_kernel(RescueArgs a)
{
    constexpr int C = LQ / 64;
    static_assert(LQ % 64 == 0 && C <= 4 && LQ <= kAlignMaxLen, "2 bits of column inside a lane");
    __shared__ __align__(16) uint8_t wbuf[kRescueMaxRows];
    __shared__ __align__(16) uint8_t qbuf[kAlignMaxLen];
    const int lane = threadIdx.x;
    const int match = a.match, mismatch = a.mismatch, ext = a.gap_extend, open_ext = a.gap_open + a.gap_extend;

    for (int64_t p = blockIdx.x; p < a.ntasks; p += gridDim.x) {
        // ---- the task's region and query, the same on every lane
        const GenomeRegion rg = rescue_region(a.anchor_ids[p], a.glen, a.ref_len, a.dlo, a.dhi);
        const int n = min(max(rg.len, 0), kRescueMaxRows);
        int m;
        const uint8_t *qp = query_row(a, a.task_query[p], LQ, m);
        // rows run over the region as oriented: genome[start + r] forward, comp(genome[start + len - 1 - r]) reversed
        const uint8_t *gp = a.genome + rg.start + (rg.reverse ? rg.len - 1 : 0);
        const int dir = rg.reverse ? -1 : 1;
        __syncthreads(); // the previous task's step loop has read its LDS
        // four coalesced byte loads in flight per lane and trip (a 1,000-row region is four trips)
        for (int r0 = lane; r0 < n; r0 += 256) {
            int v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                v[u] = r0 + 64 * u < n ? (int)gp[(r0 + 64 * u) * dir] : 0;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (r0 + 64 * u < n)
                    wbuf[r0 + 64 * u] = (uint8_t)(rg.reverse ? comp_byte(v[u]) : v[u]);
        }
        for (int j = lane; j < m; j += 64)
            qbuf[j] = qp[j];
        __syncthreads();

        // ---- DP: H and F of the lane's C columns for the previous row in registers
        int qv[C], H[C], F[C];
        uint32_t cellkey[C];
        column_setup<C>(qbuf, m, lane, qv, cellkey);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            H[c] = 0;
            F[c] = kNegInf;
        }
        // the left neighbour's last column: H of this row and of the row above, E of this row
        int left_cur = 0, left_prev = 0, left_e = kNegInf, e_last = kNegInf;
        uint32_t best = 0;
        const int steps = skew_steps<C>(n, m);
        for (int t = 0; t < steps; ++t) {
            const int i0 = t - lane;
            if (i0 >= 0 && i0 < n) {
                const int wb = wbuf[i0];
                int diag = left_prev, left = left_cur, e = left_e;
                uint32_t rowbest = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int up = H[c];
                    const int f = max(up - open_ext, F[c] - ext);
                    e = max(left - open_ext, e - ext);
                    const int h = max(max(max(diag + (wb == qv[c] ? match : -mismatch), f), e), 0);
                    rowbest = max(rowbest, ((uint32_t)h << RescueKey::kHShift) | cellkey[c]);
                    diag = up;
                    left = h;
                    H[c] = h;
                    F[c] = f;
                }
                e_last = e;
                best = max(best, rowbest | RescueKey::row(i0));
            }
            // a lane that has not started yet still holds H = 0 and E = -inf: the borders above row 0; lane 0's left
            // neighbour is column 0, H = 0 and E = -inf on every row
            left_prev = left_cur;
            left_cur = shift_up1(0, H[C - 1]);
            left_e = shift_up1(kNegInf, e_last);
        }
        best = wave_max_u32(best);

        // ---- the record, the same on every lane
        const int score = RescueKey::score(best);
        drm_rescue_result r;
        r.region_start = rg.start;
        r.region_len = rg.len;
        r.reverse = rg.reverse;
        r.score = score;
        r.ref_end = score > 0 ? RescueKey::i_end(best) : 0;
        r.q_end = score > 0 ? RescueKey::j_end<C>(best) : 0;
        r.status = score > 0 ? 0 : 1;
        if (lane == 0)
            a.out[p] = r;
    }
}

} // namespace

void launch_mate_rescue(int device, const RescueArgs &a, int max_qlen, hipStream_t stream)
{
    if (a.ntasks <= 0)
        return;
    if (max_qlen > kAlignMaxLen)
        throw Error(DRM_ERR_UNSUPPORTED, "query length " + std::to_string(max_qlen) +
                                             " > 256 is not supported by the GPU mate rescue kernel");
    if (a.dhi - a.dlo + a.ref_len > kRescueMaxRows)
        throw Error(DRM_ERR_UNSUPPORTED, "a rescue region of " + std::to_string(a.dhi - a.dlo + a.ref_len) +
                                             " > 2048 rows is not supported by the GPU mate rescue kernel");
    const bool cols3 = max_qlen <= 192; // 150 bp reads + "<" ">" tags: 3 columns per lane
    void (*kernel)(RescueArgs) = cols3 ? mate_rescue_kernel<192> : mate_rescue_kernel<256>;
    int cus = 0;
    DRM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    // bounded grid, each wave loops over tasks: 2.3 KB of LDS per wave never limits, and at 41 / 47 VGPRs the registers
    // allow the CU's full 32 waves (8 per SIMD), which hide the dependent chain through a lane's cells. A multiple of the
    // CU's 4 SIMDs, because the kernel is bound by VALU issue and the static loop gives every wave the same number of
    // tasks: a SIMD with one wave more than the others would set the time
    constexpr int per_cu = 32;
    const int grid = (int)std::min<int64_t>(a.ntasks, (int64_t)std::max(cus, 1) * per_cu);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), 0, stream, a);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
