// deepreadmapper_amd/csrc/sw_md.hip -- the MD words of aligned pairs, for gfx950.
//
// The SAM MD tag says which reference bases an alignment's mismatching and deleted columns hold. The aligners
// (sw_align.hip, sw_align_affine.hip) leave a record and run-length operation words per pair; this pass walks them
// over the same region and query bytes and writes the token stream that include/drm_hip.h defines (drm_sw_align_md):
// numbers of matching columns, mismatch words and deleted-base words.
//
// Mapping: one wave per pair, nothing serial in the number of columns.
//   1. Lane l loads the operation words [8 l, 8 l + 8), sums their reference and query spans, and a wave prefix sum
//      gives every operation its start on both strings; the totals and the words' kinds and lengths are checked here
//      (status 3). Each operation then goes to LDS as one packed word (start on the region, start on the query, kind).
//   2. Lane l owns the reference columns [4 l, 4 l + 4) of the alignment. A column finds its operation by a binary
//      search over the packed words' region starts, reads its region byte and, in an M operation, its query byte
//      straight from global memory (every byte is needed once), and is a match, a mismatch, the first byte of a D
//      operation or a later one. A mismatch and a D operation's first byte put a number in front of their own word.
//   3. One wave prefix sum over (words, matches, mismatches) places every word; a running maximum over "matches in
//      front of the latest column that wrote a number" turns the match prefix into the run lengths.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sw_wave.h"

namespace drm {
namespace {

constexpr int kOpsPerLane = kMdMaxOps / 64;    // 8
constexpr int kColsPerLane = kAlignMaxLen / 64; // 4
constexpr int kLenCap = kAlignMaxLen + 1;       // a longer operation cannot fit: summed as this, which fails the span check

// inclusive wave scans, lane 0 first
__device__ __forceinline__ int wave_scan_add(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off);
        v += lane >= off ? t : 0;
    }
    return v;
}
__device__ __forceinline__ int wave_scan_max(int v, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off);
        v = lane >= off ? max(v, t) : v;
    }
    return v;
}

// column classes
enum : int { kMatch = 0, kMismatch = 1, kDelFirst = 2, kDelNext = 3 };

__global__ __launch_bounds__(64) void sw_md_kernel(MdArgs ma)
{
    const AlignArgs &a = ma.base;
    // one packed word per operation: region start (9 bits) | query start << 9 (9 bits) | kind << 18
    __shared__ uint32_t optab[kMdMaxOps];
    const int lane = threadIdx.x;

    for (int64_t p = blockIdx.x; p < a.npairs; p += gridDim.x) {
        // ---- the pair's region and query
        const uint64_t wid = a.window_ids[p];
        const int64_t qi = a.pair_query[p]; // both indices are on their way before either is used
        const WaveRegion rg = align_region(a, wid, ma.flank);
        const int n = rg.len;
        int m;
        const uint8_t *qp = query_row(a, qi, kAlignMaxLen, m);

        // ---- what the record alone decides; every lane holds the same values
        const drm_sw_alignment r = ma.rec[p];
        int status = 0;
        if (r.status == 1 || n == 0 || m == 0)
            status = 1;
        else if (r.status != 0 || r.n_ops < 1 || r.n_ops > kMdMaxOps || r.ref_begin < 0 || r.q_begin < 0 ||
                 r.ref_begin > r.ref_end || r.ref_end > n || r.q_begin > r.q_end || r.q_end > m)
            status = 3;
        status = __builtin_amdgcn_readfirstlane(status);
        const int nops = status == 0 ? __builtin_amdgcn_readfirstlane(r.n_ops) : 0; // no word is read otherwise
        const int R = r.ref_end - r.ref_begin, Q = r.q_end - r.q_begin;

        // ---- 1. the operations: spans, checks, starts
        uint32_t w[kOpsPerLane];
        int rsum = 0, qsum = 0, bad = 0;
        const uint32_t *op = ma.ops + ma.ops_off[p];
#pragma unroll
        for (int i = 0; i < kOpsPerLane; ++i) {
            const int x = lane * kOpsPerLane + i;
            w[i] = 0;
            if (x < nops) {
                w[i] = op[x];
                const uint32_t kind = w[i] & 15u;
                const int len = (int)min(w[i] >> 4, (uint32_t)kLenCap);
                bad |= kind > 2u || len == 0;
                rsum += kind != 1u ? len : 0; // M and D consume region bytes
                qsum += kind != 2u ? len : 0; // M and I consume query bytes
            }
        }
        const int rincl = wave_scan_add(rsum, lane), qincl = wave_scan_add(qsum, lane);
        const int rtotal = __shfl(rincl, 63), qtotal = __shfl(qincl, 63);
        if (status == 0 && (__ballot(bad) != 0ull || rtotal != R || qtotal != Q))
            status = 3;
        __syncthreads(); // the previous pair's columns have read the table
        if (status == 0) { // every start is at most 256 now
            int rs = rincl - rsum, qs = qincl - qsum;
#pragma unroll
            for (int i = 0; i < kOpsPerLane; ++i) {
                const int x = lane * kOpsPerLane + i;
                if (x < nops) {
                    const uint32_t kind = w[i] & 15u;
                    const int len = (int)(w[i] >> 4);
                    optab[x] = (uint32_t)rs | ((uint32_t)qs << 9) | (kind << 18);
                    rs += kind != 1u ? len : 0;
                    qs += kind != 2u ? len : 0;
                }
            }
        }
        __syncthreads();

        // ---- 2. the columns: class and region byte of each, the lane's sums
        const int ncols = status == 0 ? R : 0;
        int cls[kColsPerLane], base[kColsPerLane];
        int sums = 0; // words | matches << 10 | mismatches << 19: at most 512, 256 and 256
#pragma unroll
        for (int i = 0; i < kColsPerLane; ++i) {
            const int c = lane * kColsPerLane + i;
            cls[i] = -1;
            base[i] = 0;
            if (c < ncols) {
                // the last operation that starts at or before c: it consumes region bytes, an I operation sharing
                // its start with the operation behind it; optab[0] starts at 0
                int lo = 0;
#pragma unroll
                for (int step = kMdMaxOps / 2; step > 0; step >>= 1)
                    if (lo + step < nops && (int)(optab[lo + step] & 511u) <= c)
                        lo += step;
                const uint32_t e = optab[lo];
                const int rstart = (int)(e & 511u), qstart = (int)((e >> 9) & 511u);
                const int ri = r.ref_begin + c; // < ref_end <= n
                base[i] = rg.byte(ri);
                if ((e >> 18) == 0u) {
                    const int qj = r.q_begin + qstart + (c - rstart); // < q_end <= m: the spans were checked
                    cls[i] = base[i] == (int)qp[qj] ? kMatch : kMismatch;
                } else {
                    cls[i] = c == rstart ? kDelFirst : kDelNext;
                }
                sums += cls[i] == kMatch ? 1 << 10 : cls[i] == kMismatch ? 2 + (1 << 19) : cls[i] == kDelFirst ? 2 : 1;
            }
        }

        // ---- 3. positions and run lengths
        const int incl = wave_scan_add(sums, lane);
        const int total = __shfl(incl, 63);
        int before = incl - sums; // words and matches in front of the lane's first column
        // matches in front of the latest column that wrote a number, 0 when there is none: the match prefix never
        // falls, so that is a maximum
        int flushed[kColsPerLane], lane_max = 0, at = before;
#pragma unroll
        for (int i = 0; i < kColsPerLane; ++i) {
            flushed[i] = lane_max;
            const int matches = (at >> 10) & 511;
            if (cls[i] == kMismatch || cls[i] == kDelFirst)
                lane_max = max(lane_max, matches);
            at += cls[i] == kMatch ? 1 << 10 : cls[i] == kMismatch ? 2 : cls[i] == kDelFirst ? 2 : cls[i] == kDelNext ? 1 : 0;
        }
        const int max_incl = wave_scan_max(lane_max, lane);
        const int max_before = shift_up1(0, max_incl);
        const int max_total = __shfl(max_incl, 63);

        uint32_t *out = ma.md + p * (int64_t)ma.md_stride;
        at = before;
#pragma unroll
        for (int i = 0; i < kColsPerLane; ++i) {
            int pos = at & 1023;
            const int matches = (at >> 10) & 511;
            if (cls[i] == kMismatch || cls[i] == kDelFirst) {
                if (pos < ma.md_stride)
                    out[pos] = (uint32_t)(matches - max(max_before, flushed[i])) << 4;
                ++pos;
            }
            if (cls[i] > kMatch && pos < ma.md_stride)
                out[pos] = ((uint32_t)base[i] << 4) | (cls[i] == kMismatch ? 1u : 2u);
            at += cls[i] == kMatch ? 1 << 10 : cls[i] == kMismatch ? 2 : cls[i] == kDelFirst ? 2 : cls[i] == kDelNext ? 1 : 0;
        }
        if (lane == 0) {
            drm_sw_md h = {0, 0, 0, 0, 0, status};
            if (status == 0) {
                const int words = total & 1023, matches = (total >> 10) & 511, mismatches = (total >> 19) & 511;
                if (words < ma.md_stride) // the number behind the last operation
                    out[words] = (uint32_t)(matches - max_total) << 4;
                h.n_words = words + 1;
                h.n_match = matches;
                h.n_mismatch = mismatches;
                h.n_ins = Q - matches - mismatches; // what the M columns leave of the query span: the I operations
                h.n_del = R - matches - mismatches;
                h.status = h.n_words > ma.md_stride ? 2 : 0;
            }
            ma.out[p] = h;
        }
    }
}

} // namespace

void launch_sw_md(const DeviceRefs &refs, const MdArgs &ma, int max_qlen, hipStream_t stream)
{
    if (ma.base.npairs <= 0)
        return;
    check_align_launch("MD", refs.ref_len, ma.flank, max_qlen);
    int cus = 0;
    DRM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, refs.device));
    // the pass waits on memory, not on issue: 16 one-wave blocks a CU (4 per SIMD) to hide it, each looping over pairs
    const int grid = (int)std::min<int64_t>(ma.base.npairs, (int64_t)std::max(cus, 1) * 16);
    hipLaunchKernelGGL(sw_md_kernel, dim3(grid), dim3(64), 0, stream, ma);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
