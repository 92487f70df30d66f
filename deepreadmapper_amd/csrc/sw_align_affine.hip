// deepreadmapper_amd/csrc/sw_align_affine.hip -- affine-gap Smith-Waterman alignment with traceback over a flanked
// genome region, for gfx950.
//
// The alignment that gets printed (DRM_SAM_CIGAR with DRM_SAM_SCORING / DRM_SAM_FLANK): Gotoh's recurrence with the
// caller's match / mismatch / gap-open / gap-extend scores over the hit's window widened by `flank` genome bases on
// either side, as defined in include/drm_hip.h (drm_sw_align_affine). The linear kernel (sw_align.hip) stays the
// rerank's alignment; at {1, 1, 0, 1} and flank 0 the two definitions coincide.
//
// Mapping: that of sw_align.hip -- one wave per pair, lane l owns the C = LQ / 64 query
// columns [l * C, l * C + C), rows skewed by lane -- with F (the gap that runs down a column) in registers beside H,
// and E (the gap that runs along a row) carried through the lane's columns and handed to the right neighbour together
// with H, each in one DPP shift per step. A cell's direction is 4 bits (source of H, "F extended", "E extended"), so a
// lane writes one 16-bit word per row, [row][lane] over the lanes that hold a query column (102 B per row for 152-byte
// reads); the traceback runs from LDS in the same kernel.
//
// The end-aware instantiation (CLIP, drm_sw_align_affine_clip) is the same loop with the floor of
// H a per-column register instead of the constant 0 and the end term of the clipping penalty folded into the best-cell
// key; the plain instantiation compiles to what it was.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sw_wave.h"

namespace drm {
namespace {

// Every value is kept times 4. H is one signed maximum over its candidates in the form 4 * value + priority
// (M 2, F 1, E 0), floored at 3 = "H is 0: the walk stops", exactly as in sw_align.hip. F and E are a maximum over
// 4 * (H - open - ext) + 1 and 4 * (F or E - ext): bit 0 of the winner says "the gap was opened here", and an equal
// pair is won by the opening, which is the definition's "closing wins a tie against extending" seen from the walk.
enum : uint32_t { kSrcE = 0, kSrcF = 1, kSrcM = 2, kSrcStop = 3, kFExt = 4, kEExt = 8 };

constexpr int kNegInf = -(1 << 20); // the borders' E and F: below every real value, far from overflow, 0 mod 4

// LDS: ops[kOpsWords] u32 | region[256] | query[256] | dirs[n][dir_lanes] u16
constexpr size_t kAffineLdsFixed = sizeof(uint32_t) * kOpsWords + 2 * kAlignMaxLen;

template <int LQ, bool CLIP>
__global__ __launch_bounds__(64) void sw_align_affine_kernel(AffineAlignArgs aa)
{
    constexpr int C = LQ / 64;
    static_assert(LQ % 64 == 0 && 4 * C <= 16, "one 16-bit direction word per lane and row");
    const AlignArgs &a = aa.base;
    extern __shared__ __align__(16) uint8_t smem[];
    uint32_t *opsbuf = reinterpret_cast<uint32_t *>(smem);
    uint8_t *wbuf = smem + sizeof(uint32_t) * kOpsWords;
    uint8_t *qbuf = wbuf + kAlignMaxLen;
    uint16_t *dirs = reinterpret_cast<uint16_t *>(qbuf + kAlignMaxLen);
    const int lane = threadIdx.x;
    const int dir_lanes = aa.dir_lanes; // every query column lies on a lane below it: the launch's ceil(max_qlen / C)
    const int match4 = 4 * aa.match, mismatch4 = 4 * aa.mismatch, ext4 = 4 * aa.gap_extend;
    const int open4 = 4 * (aa.gap_open + aa.gap_extend) - 1; // H - open4 = 4 * (H - open - ext) + 1
    // CLIP: the read is columns a + 1 .. b (1-based) of the query, b from the pair's own length; an alignment that
    // starts right of a or ends off b pays clip4 / 4. Keys carry the adjusted score plus kKeyBias, so that the packed
    // unsigned key stays monotone below 0: adjusted values lie in [-126, 31 * 256].
    constexpr int kKeyBias = CLIP ? 128 : 0;
    const int clip4 = CLIP ? 4 * aa.clip_penalty : 0;
    const int tag_a = CLIP ? aa.tag_prefix : 0;

    for (int64_t p = blockIdx.x; p < a.npairs; p += gridDim.x) {
        // ---- the pair's region and query
        const uint64_t wid = a.window_ids[p];
        const int64_t qi = a.pair_query[p]; // both indices are on their way before either is used
        const WaveRegion rg = align_region(a, wid, aa.flank);
        const int n = rg.len;
        int m;
        const uint8_t *qp = query_row(a, qi, LQ, m);
        const int tag_b = m - (CLIP ? aa.tag_postfix : 0);
        if (CLIP && tag_b < tag_a) // no read between the tags: no alignment
            m = 0;
        __syncthreads(); // the previous pair's traceback has read its LDS
        stage_region(wbuf, rg, lane);

        // ---- DP: 4 * H and 4 * F of the lane's C columns for the previous row in registers
        int qv[C], H4[C], F4[C];
        int stop4[C], end4[C]; // CLIP: 4 * floor(j) + 3, and 4 * kKeyBias less the column's end term
        uint32_t cellkey[C];
        column_setup<C>(qp, m, lane, qv, cellkey);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j0 = lane * C + c;
            if (j0 < m)
                qbuf[j0] = (uint8_t)qv[c];
            stop4[c] = CLIP && j0 >= tag_a ? (int)kSrcStop - clip4 : (int)kSrcStop; // column j0 + 1 > a
            end4[c] = 4 * kKeyBias - (j0 + 1 == tag_b ? 0 : clip4);
            H4[c] = stop4[c] - (int)kSrcStop; // row 0: H = floor(j)
            F4[c] = kNegInf;
        }
        __syncthreads();
        // the left neighbour's last column: 4 * H of this row and of the row above, 4 * E of this row
        // (rows 0 and -1 of the column left of the lane's first: its floor; column 0 is 0 on every row)
        const int left0 = CLIP && lane * C > tag_a ? -clip4 : 0;
        int left_cur = left0, left_prev = left0, left_e = kNegInf, e_last = kNegInf;
        // the best cell's AlignKey. CLIP: of H less the end term plus kKeyBias, still < 2^13
        uint32_t best = 0;
        const int steps = skew_steps<C>(n, m);
        for (int t = 0; t < steps; ++t) {
            const int i0 = t - lane;
            if (i0 >= 0 && i0 < n) {
                const int wb = wbuf[i0];
                int diag = left_prev, left = left_cur, e = left_e;
                uint32_t dbits = 0, rowbest = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int up = H4[c];
                    const int fk = max(up - open4, F4[c] - ext4);
                    const int ek = max(left - open4, e - ext4);
                    const int f = fk & ~1;
                    e = ek & ~1;
                    const int km = diag + (wb == qv[c] ? match4 : -mismatch4) + (int)kSrcM;
                    const uint32_t k = (uint32_t)max(max(max(km, f + (int)kSrcF), e + (int)kSrcE),
                                                     CLIP ? stop4[c] : (int)kSrcStop);
                    // bit 0 of fk / ek set = opened: "extended" is its complement, at bits 2 and 3
                    dbits |= ((k & 3u) | ((uint32_t)(~fk & 1) << 2) | ((uint32_t)(~ek & 1) << 3)) << (4 * c);
                    const uint32_t h4 = k & ~3u;
                    rowbest = max(rowbest, ((CLIP ? h4 + (uint32_t)end4[c] : h4) << (AlignKey::kHShift - 2)) | cellkey[c]);
                    diag = up;
                    left = (int)h4;
                    H4[c] = (int)h4;
                    F4[c] = f;
                }
                e_last = e;
                best = max(best, rowbest | AlignKey::row(i0));
                if (lane < dir_lanes) // the lanes past it hold padded columns only, which the walk never visits
                    dirs[i0 * dir_lanes + lane] = (uint16_t)dbits;
            }
            // a lane that has not started yet still holds H = 0 and E = -inf: the borders above row 0; lane 0's left
            // neighbour is column 0, H = 0 and E = -inf on every row
            left_prev = left_cur;
            left_cur = shift_up1(0, H4[C - 1]);
            left_e = shift_up1(kNegInf, e_last);
        }
        best = wave_max_u32(best);
        __syncthreads(); // every direction word is in LDS

        // ---- traceback: every lane walks the same path (LDS broadcasts), so no lane-0 branch surrounds the loop.
        //      state 0 = H, 1 = F (a run of region bytes, D), 2 = E (a run of query bytes, I)
        const int adj = AlignKey::score(best) - kKeyBias; // the plain score; CLIP: less the end term (no cell: -128)
        int score = CLIP ? max(adj, 0) : adj;
        const int i_end = score > 0 ? AlignKey::i_end(best) : 0;
        const int j_end = score > 0 ? AlignKey::j_end<C>(best) : 0;
        int i = i_end, j = j_end, nm = 0, state = 0;
        RunWriter runs{opsbuf};
        while (i > 0 && j > 0) {
            const int col = j - 1, ln = col / C, c = col - ln * C;
            const uint32_t d = ((uint32_t)dirs[(i - 1) * dir_lanes + ln] >> (4 * c)) & 15u;
            int move = state; // 1 = D, 2 = I, 3 = M
            if (state == 0) {
                const uint32_t src = d & 3u;
                if (src == kSrcStop)
                    break;
                move = src == kSrcM ? 3 : src == kSrcF ? 1 : 2;
            }
            uint32_t op; // BAM: M 0, I 1, D 2
            if (move == 3) {
                op = 0u;
                nm += wbuf[i - 1] != qbuf[j - 1];
                --i;
                --j;
                state = 0;
            } else if (move == 1) {
                op = 2u;
                ++nm;
                state = (d & kFExt) ? 1 : 0;
                --i;
            } else {
                op = 1u;
                ++nm;
                state = (d & kEExt) ? 2 : 0;
                --j;
            }
            runs.step(op);
        }
        runs.finish();
        __syncthreads();
        runs.store_reversed(a, p, lane);
        if (CLIP && score > 0) // the plain affine score of the walk: what it paid for its two ends comes back
            score += (j > tag_a ? clip4 / 4 : 0) + (j_end != tag_b ? clip4 / 4 : 0);
        store_alignment(a, p, lane, score, i, i_end, j, j_end, nm, runs.nops);
    }
}

} // namespace

void launch_sw_align_affine(const DeviceRefs &refs, AffineAlignArgs aa, int max_qlen, hipStream_t stream)
{
    if (aa.base.npairs <= 0)
        return;
    const int region = refs.ref_len + 2 * aa.flank;
    check_align_launch("affine SW alignment", refs.ref_len, aa.flank, max_qlen);
    int cus = 0;
    DRM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, refs.device));
    // one direction word per row for each lane that can hold a query column
    const int cols = max_qlen <= 192 ? 3 : 4; // 150 bp reads + "<" ">" tags: 3 columns per lane
    aa.dir_lanes = std::max((max_qlen + cols - 1) / cols, 1);
    // bounded grid, each wave loops over pairs: as many waves per CU as its 160 KB of LDS hold (152-byte reads: 17.4 KB
    // each at 150-byte windows: 9; 19.0 KB at flank 8: 8; 256 x 256 bytes, 34.5 KB: 4), 16 at the most, rounded down to
    // a multiple of the CU's 4 SIMDs. The kernel is bound by VALU issue and every wave takes the same number of pairs,
    // so a SIMD with one wave more than the others sets the time: 9 per CU measured slower than 8.
    const size_t lds = kAffineLdsFixed + (size_t)std::max(region, 1) * aa.dir_lanes * sizeof(uint16_t);
    const int per_cu = (int)std::min<size_t>(16, (size_t)160 * 1024 / lds) & ~3; // lds <= 34.5 KB: at least 4
    const int grid = (int)std::min<int64_t>(aa.base.npairs, (int64_t)std::max(cus, 1) * per_cu);
    auto kernel = cols == 3 ? (aa.end_aware ? sw_align_affine_kernel<192, true> : sw_align_affine_kernel<192, false>)
                            : (aa.end_aware ? sw_align_affine_kernel<256, true> : sw_align_affine_kernel<256, false>);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64), lds, stream, aa);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
