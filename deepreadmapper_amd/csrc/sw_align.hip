// deepreadmapper_amd/csrc/sw_align.hip -- Smith-Waterman alignment with traceback for gfx950.
//
// The score kernel (sw_rerank.hip) keeps only the best score. This kernel reruns the full DP of
// calc_sw_score (src/utils/metrics.cpp:10-45) for the pairs that get printed, records a direction per cell
// and walks it back: the reference leaves this open ("TODO: Implement real CIGAR - from SW ranker",
// src/utils/utils.cpp:380-384), so the alignment is the one defined in include/drm_hip.h (drm_sw_align).
//
// Mapping: one wave per pair. Lane l owns the C = LQ / 64 query columns
// [l * C, l * C + C); rows are skewed, at step t lane l works on window row t - l, so a pair takes
// n + ceil(m / C) - 1 steps. The only value that crosses lanes is the left neighbour's last-column H of the row the lane works
// on next; it moves one lane up per step in a DPP shift. Directions take 2 bits per cell, one byte per lane
// and row in LDS ([row][lane], 64 B per row); the traceback runs from LDS in the same kernel.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sw_wave.h"

namespace drm {
namespace {

// A cell is one signed maximum over its three candidates in the form 4 * H + priority (M 2, D 1, I 0), floored at
// 3 = "H is 0: the walk stops": the result's upper bits are 4 * H and its low two bits are the direction, with the
// definition's order of preference (M, then D, then I) settled by the same maximum.
enum : uint32_t { kDirI = 0, kDirD = 1, kDirM = 2, kDirStop = 3 };

// LDS: ops[kOpsWords] u32 | window[256] | dirs[ref_len][64]
constexpr size_t kAlignLdsFixed = sizeof(uint32_t) * kOpsWords + kAlignMaxLen;

template <int LQ>
__global__ __launch_bounds__(64) void sw_align_kernel(AlignArgs a)
{
    constexpr int C = LQ / 64;
    static_assert(LQ % 64 == 0 && 2 * C <= 8, "one direction byte per lane and row");
    extern __shared__ __align__(16) uint8_t smem[];
    uint32_t *opsbuf = reinterpret_cast<uint32_t *>(smem);
    uint8_t *wbuf = smem + sizeof(uint32_t) * kOpsWords;
    uint8_t *dirs = wbuf + kAlignMaxLen;
    const int lane = threadIdx.x;

    for (int64_t p = blockIdx.x; p < a.npairs; p += gridDim.x) {
        // ---- the pair's window (the region at flank 0) and query
        const uint64_t wid = a.window_ids[p];
        const int64_t qi = a.pair_query[p]; // both indices are on their way before either is used
        const WaveRegion rg = align_region(a, wid, 0);
        const int n = rg.len;
        int m;
        const uint8_t *qp = query_row(a, qi, LQ, m);
        __syncthreads(); // the previous pair's traceback has read its LDS
        stage_region(wbuf, rg, lane);
        __syncthreads();

        // ---- DP: 4 * H of the lane's C columns for the previous row in registers
        int qv[C], H4[C] = {};
        uint32_t cellkey[C];
        column_setup<C>(qp, m, lane, qv, cellkey);
        int left_cur = 0, left_prev = 0; // 4 * H of the left neighbour's last column: this row, the row above
        uint32_t best = 0;               // the best cell's AlignKey
        const int steps = skew_steps<C>(n, m);
        for (int t = 0; t < steps; ++t) {
            const int i0 = t - lane;
            if (i0 >= 0 && i0 < n) {
                const int wb = wbuf[i0];
                int diag = left_prev, left = left_cur;
                uint32_t dbits = 0, rowbest = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int up = H4[c];
                    const int km = diag + (wb == qv[c] ? 4 + (int)kDirM : -4 + (int)kDirM);
                    const int kd = up - 4 + (int)kDirD, ki = left - 4 + (int)kDirI;
                    const uint32_t k = (uint32_t)max(max(max(km, kd), ki), (int)kDirStop);
                    dbits |= (k & 3u) << (2 * c);
                    const uint32_t h4 = k & ~3u;
                    rowbest = max(rowbest, (h4 << (AlignKey::kHShift - 2)) | cellkey[c]);
                    diag = up;
                    left = (int)h4;
                    H4[c] = (int)h4;
                }
                best = max(best, rowbest | AlignKey::row(i0));
                dirs[i0 * 64 + lane] = (uint8_t)dbits;
            }
            // a lane that has not started yet still holds H = 0: the zero border above row 0
            left_prev = left_cur;
            left_cur = shift_up1(0, H4[C - 1]);
        }
        best = wave_max_u32(best);
        __syncthreads(); // every direction byte is in LDS

        // ---- traceback: every lane walks the same path (LDS broadcasts), so no lane-0 branch surrounds the loop
        const int score = AlignKey::score(best);
        const int i_end = score > 0 ? AlignKey::i_end(best) : 0;
        const int j_end = score > 0 ? AlignKey::j_end<C>(best) : 0;
        int i = i_end, j = j_end, n_m = 0, n_gap = 0;
        RunWriter runs{opsbuf};
        while (i > 0 && j > 0) {
            const int col = j - 1, ln = col / C, c = col - ln * C;
            const uint32_t d = ((uint32_t)dirs[(i - 1) * 64 + ln] >> (2 * c)) & 3u;
            if (d == kDirStop)
                break;
            const uint32_t op = d == kDirM ? 0u : d == kDirD ? 2u : 1u; // BAM: M 0, I 1, D 2
            n_m += d == kDirM;
            n_gap += d != kDirM;
            if (d != kDirI)
                --i;
            if (d != kDirD)
                --j;
            runs.step(op);
        }
        runs.finish();
        __syncthreads();
        runs.store_reversed(a, p, lane);
        // score = matches - mismatches - gap bases and n_m = matches + mismatches
        store_alignment(a, p, lane, score, i, i_end, j, j_end, n_gap + (n_m - n_gap - score) / 2, runs.nops);
    }
}

} // namespace

void launch_sw_align(const DeviceRefs &refs, AlignArgs a, int max_qlen, hipStream_t stream)
{
    if (a.npairs <= 0)
        return;
    check_align_launch("SW alignment", refs.ref_len, 0, max_qlen);
    int cus = 0;
    DRM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, refs.device));
    // bounded grid, each wave loops over pairs: 16 waves per CU (11.6 KB of LDS each at 150-byte windows)
    const int grid = (int)std::min<int64_t>(a.npairs, (int64_t)std::max(cus, 1) * 16);
    const size_t lds = kAlignLdsFixed + (size_t)std::max(refs.ref_len, 1) * 64;
    if (max_qlen <= 192) // 150 bp reads + "<" ">" tags: 3 columns per lane
        hipLaunchKernelGGL(sw_align_kernel<192>, dim3(grid), dim3(64), lds, stream, a);
    else
        hipLaunchKernelGGL(sw_align_kernel<256>, dim3(grid), dim3(64), lds, stream, a);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
