// deepreadmapper_amd/csrc/locus_scan.h -- the locus scan of one staged hit list, shared by the kernels that run it
// (mapq.hip: hit_mapq_kernel, pair_mapq_kernel; tlen_scan.hip: tlen_scan_kernel), and their grid rule.
//
// A list is staged in LDS as (window id u64, one state word), row i held by lane i & 63. The state word is the score
// (21 bits) with two flags above it: bit 31 "removed" (dead rows are staged removed) and bit 30 "in locus 0". One scan
// iteration is one pass of every lane over its own rows: the rows in the locus of the current head are marked removed by
// one unsigned 64-bit range compare, (pos - (hpos - (span - 1))) <= 2 * (span - 1) (positions are below 2^63 and
// span <= 2^20, so the difference mod 2^64 falls into the range only when it is in it), and the same pass takes the
// maximum of score << 10 | (1023 - i) over the rows that remain: the next head and its tie rule at once, reduced by one
// butterfly. Every iteration removes at least its own head, so the scan ends after at most `count` iterations, and the
// loop is bounded by that count as well. The lanes only ever write their own rows; the head's id is a wave-uniform LDS
// read.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "drm_device.h"

namespace drm {
namespace {

constexpr uint32_t kRemoved = 1u << 31, kLocus0 = 1u << 30, kScoreMask = (1u << 21) - 1;
static_assert(kMaxCands <= 1024, "the row takes 10 bits of the scan's key");

__device__ __forceinline__ uint32_t wave_max32(uint32_t x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        x = max(x, (uint32_t)__shfl_xor((int)x, off));
    return x;
}

// rows [0, c) of one list into LDS; returns the wave's top key, score << 10 | (1023 - i) of the top live row, or 0
__device__ __forceinline__ uint32_t stage_list(const uint64_t *ids, const int32_t *scores, int c, int lane,
                                               uint64_t *lid, uint32_t *lst)
{
    uint32_t top = 0;
    for (int base = 0; base < c; base += 64) {
        const int i = base + lane;
        if (i < c) {
            const int32_t s = scores[i];
            const uint32_t sm = s > 0 ? (uint32_t)s & kScoreMask : 0u; // scores beyond 2^20 break the contract
            lid[i] = ids[i];
            lst[i] = sm ? sm : kRemoved;
            top = max(top, sm ? (sm << 10) | (uint32_t)(1023 - i) : 0u);
        }
    }
    return wave_max32(top);
}

// marks every remaining row in the locus of id hw with `mark` (which holds kRemoved), counts them, and returns the
// top key of the rows that remain
__device__ __forceinline__ uint32_t remove_locus(const uint64_t *lid, uint32_t *lst, int c, int lane, uint64_t hw,
                                                 uint64_t span_m1, uint32_t mark, int &removed)
{
    const uint64_t edge = (hw >> 1) - span_m1;
    uint32_t top = 0;
    for (int base = 0; base < c; base += 64) {
        const int i = base + lane;
        const bool held = i < c;
        const uint32_t v = held ? lst[i] : kRemoved;
        const uint64_t w = held ? lid[i] : 0;
        const bool in_play = !(v & kRemoved);
        const bool same = in_play && ((w ^ hw) & 1u) == 0 && ((w >> 1) - edge) <= 2 * span_m1;
        if (same)
            lst[i] = v | mark;
        removed += __popcll(__ballot(same));
        const uint32_t key = (in_play && !same) ? ((v & kScoreMask) << 10) | (uint32_t)(1023 - i) : 0u;
        top = max(top, key);
    }
    return wave_max32(top);
}

struct LocusScan {
    int best, best_score, locus_rows, sub_row, sub_score, n_sub, status;
};

// The locus scan of the staged list (drm_hip.h) with head row `head` (wave-uniform; -1 = the row of `top`, the list's
// top key). Every value here is wave-uniform. Leaves locus 0's rows marked kLocus0.
__device__ __forceinline__ LocusScan locus_scan(const uint64_t *lid, uint32_t *lst, int c, int lane, int head,
                                                uint32_t top, const drm_mapq_params &prm)
{
    LocusScan r{-1, 0, 0, -1, 0, 0, 1};
    int h = head;
    if (h == -1) {
        if (!top)
            return r;
        h = 1023 - (int)(top & 1023u);
    } else if (h < 0 || h >= c || (lst[h] & kRemoved)) {
        return r;
    }
    const uint64_t span_m1 = (uint64_t)(uint32_t)max(prm.locus_span - 1, 0);
    r.best = h;
    r.best_score = (int)(lst[h] & kScoreMask);
    r.status = 0;
    uint32_t next = remove_locus(lid, lst, c, lane, lid[h], span_m1, kRemoved | kLocus0, r.locus_rows);
    if (next) {
        r.sub_row = 1023 - (int)(next & 1023u);
        r.sub_score = (int)(next >> 10);
    }
    for (int it = 0; it < c && next != 0; ++it) { // each trip removes at least its own head
        if ((int)(next >> 10) < r.sub_score - prm.sub_band)
            break;
        ++r.n_sub;
        int unused = 0;
        next = remove_locus(lid, lst, c, lane, lid[1023 - (int)(next & 1023u)], span_m1, kRemoved, unused);
    }
    return r;
}

inline void check_k(int k, const char *what)
{
    if (k < 0 || k > kMaxCands)
        throw Error(DRM_ERR_UNSUPPORTED, "k = " + std::to_string(k) + " outside [0, 1024]: the " + what +
                                             " kernel keeps a list of the rerank's candidate cap in LDS");
}

// bounded grid, each wave loops over its items: as many waves per CU as its 160 KB of LDS hold, 32 at the most, from 8
// on a multiple of the 4 SIMDs (the grid rule of launch_pair_hits). Below 8 every wave counts: the pair kernel's 6 at
// k = 1024 measured 35.5 ms where 4 measured 51.4
inline int bounded_grid(int64_t items, size_t lds)
{
    int dev = 0, cus = 0;
    DRM_HIP_CHECK(hipGetDevice(&dev));
    DRM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    int per_cu = (int)std::min<size_t>(32, (size_t)160 * 1024 / lds);
    per_cu = per_cu >= 8 ? per_cu & ~3 : std::max(per_cu, 4);
    return (int)std::min<int64_t>(items, (int64_t)std::max(cus, 1) * per_cu);
}

} // namespace
} // namespace drm
