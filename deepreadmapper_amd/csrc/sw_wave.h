// deepreadmapper_amd/csrc/sw_wave.h -- what the one-wave-per-pair kernels behind the printed alignment share
// (sw_align.hip, sw_align_affine.hip, sw_md.hip, mate_rescue.hip): the pair's region and query,
// the lanes' column set-up, the best-cell key, and the traceback's run writer and record. Device code only; the step
// loops, whose cells differ, stay with their kernels.
#pragma once

#include "drm_device.h"

namespace drm {

// A pair's region as a kernel reads it: `len` bytes, byte r being first[r], or the complement of first[-r]
struct WaveRegion {
    const uint8_t *first;
    int len, reverse;
    __device__ __forceinline__ int byte(int r) const { return reverse ? comp_byte(first[-r]) : (int)first[r]; }
};

// The region of window id `wid`, at most kAlignMaxLen bytes: the table row, or align_region (drm_internal.h) of the
// genome, reverse-complemented as a whole for odd ids; empty for an id outside the table and a window past the genome
// end. `flank` is 0 on a table; at flank 0 the region is the window.
__device__ __forceinline__ WaveRegion align_region(const AlignArgs &a, uint64_t wid, int flank)
{
    WaveRegion r{nullptr, 0, 0};
    if (a.genome) {
        const GenomeRegion g = align_region(wid, a.glen, a.ref_len, flank);
        if (g.len > 0)
            r = {a.genome + g.start + (g.reverse ? g.len - 1 : 0), min(g.len, kAlignMaxLen), g.reverse};
    } else if (wid < (uint64_t)a.n_ref) {
        r = {a.refs + wid * (uint64_t)a.row_stride, min(a.ref_len, kAlignMaxLen), 0};
    }
    return r;
}

// Query qi's bytes and their number m, at most `cap`; m = 0 for an index outside [0, nq)
template <class Args>
__device__ __forceinline__ const uint8_t *query_row(const Args &a, int64_t qi, int cap, int &m)
{
    m = 0;
    if (qi < 0 || qi >= a.nq)
        return nullptr;
    m = min(max(a.q_len[qi], 0), min(a.q_stride, cap));
    return a.queries + qi * (int64_t)a.q_stride;
}

// the region, oriented, into LDS
__device__ __forceinline__ void stage_region(uint8_t *wbuf, const WaveRegion &rg, int lane)
{
    for (int r = lane; r < rg.len; r += 64)
        wbuf[r] = (uint8_t)rg.byte(r);
}

// Best cell as one key, H << HShift | (kRowMax - row) << 8 | (63 - lane) << 2 | (3 - c), rows counted from RowBase:
// its maximum is the largest H, then the smallest row, then the smallest column (a smaller column is a smaller lane,
// then a smaller c). A step loop adds row(i0) to the best of H << HShift | column(lane, c) over the lane's cells.
template <int HShift, int RowBase>
struct CellKey {
    static constexpr int kHShift = HShift, kRowShift = 8, kRowMax = (1 << (HShift - kRowShift)) - 1;
    static __device__ __forceinline__ uint32_t column(int lane, int c) { return (uint32_t)(((63 - lane) << 2) | (3 - c)); }
    static __device__ __forceinline__ uint32_t row(int i0) { return (uint32_t)(kRowMax - RowBase - i0) << kRowShift; }
    static __device__ __forceinline__ int score(uint32_t k) { return (int)(k >> HShift); }
    // the cell's 1-based row and column
    static __device__ __forceinline__ int i_end(uint32_t k)
    {
        return kRowMax + 1 - RowBase - (int)((k >> kRowShift) & (uint32_t)kRowMax);
    }
    template <int C>
    static __device__ __forceinline__ int j_end(uint32_t k)
    {
        return (63 - (int)((k >> 2) & 63u)) * C + (3 - (int)(k & 3u)) + 1;
    }
};
using AlignKey = CellKey<17, 1>; // the aligners: H <= 31 * 256 < 2^13 and 9 bits of a 1-based row

// The lane's C columns [lane * C, lane * C + C) of the m query bytes q[]. -2 pads a column past the query: it matches
// no byte, and such columns lie right of every real one, which never reads them. A padded cell is some real cell's H
// minus at least its distance from it, so it never reaches the best score.
template <int C>
__device__ __forceinline__ void column_setup(const uint8_t *q, int m, int lane, int (&qv)[C], uint32_t (&cellkey)[C])
{
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j0 = lane * C + c;
        qv[c] = j0 < m ? (int)q[j0] : -2;
        cellkey[c] = AlignKey::column(lane, c); // larger = further left; the same bits under every HShift
    }
}

// rows are skewed by lane: the lane of the last real column finishes the last row at step n - 1 + (m - 1) / C
template <int C>
__device__ __forceinline__ int skew_steps(int n, int m)
{
    return (n > 0 && m > 0) ? n + (m - 1) / C : 0;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        v = max(v, (uint32_t)__shfl_xor((int)v, off));
    return v;
}

// The traceback's operations as runs, (length << 4) | BAM kind (M 0, I 1, D 2), in LDS in the order of the walk
constexpr int kOpsWords = 2 * kAlignMaxLen; // a walk has at most n + m steps, so at most as many runs
struct RunWriter {
    uint32_t *buf; // [kOpsWords]
    int nops = 0;
    uint32_t cur_op = 0, cur_len = 0;
    __device__ __forceinline__ void step(uint32_t op)
    {
        if (cur_len > 0 && op != cur_op)
            finish();
        cur_op = op;
        ++cur_len;
    }
    __device__ __forceinline__ void finish()
    {
        if (cur_len > 0)
            buf[nops++] = (cur_len << 4) | cur_op;
        cur_len = 0;
    }
    // the walk ran backwards: pair p's runs reversed, after a barrier behind the last finish()
    __device__ __forceinline__ void store_reversed(const AlignArgs &a, int64_t p, int lane) const
    {
        const int nstore = min(nops, a.ops_stride);
        for (int x = lane; x < nstore; x += 64)
            a.ops[p * (int64_t)a.ops_stride + x] = buf[nops - 1 - x];
    }
};

// pair p's record from the walk's two ends: status 1 = no alignment, 2 = more runs than ops_stride holds
__device__ __forceinline__ void store_alignment(const AlignArgs &a, int64_t p, int lane, int score, int i, int i_end,
                                                int j, int j_end, int nm, int nops)
{
    if (lane != 0)
        return;
    drm_sw_alignment r;
    r.score = score;
    r.ref_begin = i;
    r.ref_end = i_end;
    r.q_begin = j;
    r.q_end = j_end;
    r.nm = nm;
    r.n_ops = nops;
    r.status = score == 0 ? 1 : nops > a.ops_stride ? 2 : 0;
    a.out[p] = r;
}

} // namespace drm
