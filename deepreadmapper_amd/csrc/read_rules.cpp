// deepreadmapper_amd/csrc/read_rules.cpp -- the read-level rules that run on the host (include/drm_hip.h): the
// accepted ranges of the pairing, rescue, scoring and MAPQ parameters, the mate rescue's window and choice, the MAPQ
// formula's checked entry and the post-rescue MAPQ, the template-length estimate, and the duplicate marker's unclipped
// 5' end, end word and slot hash.
#include <algorithm>
#include <string>
#include <vector>

#include "drm_internal.h"

// ----------------------------------------------------------------------- mate rescue: the host-only parts
void drm::check_pair_params(const drm_pair_params *p)
{
    if (!p)
        throw Error(DRM_ERR_ARG, "null pair parameters");
    if (p->ref_len < 1 || p->ref_len > (1 << 20))
        throw Error(DRM_ERR_ARG, "ref_len " + std::to_string(p->ref_len) + " outside [1, 2^20]");
    if (p->min_tlen < 0 || p->min_tlen > p->max_tlen || p->max_tlen > (1 << 30))
        throw Error(DRM_ERR_ARG, "template lengths [" + std::to_string(p->min_tlen) + ", " +
                                     std::to_string(p->max_tlen) + "] must satisfy 0 <= min <= max <= 2^30");
}

void drm::check_rescue_params(const drm_pair_params *p, int64_t &dlo, int64_t &dhi)
{
    check_pair_params(p);
    dlo = std::max<int64_t>((int64_t)p->min_tlen - p->ref_len, 0);
    dhi = (int64_t)p->max_tlen - p->ref_len;
    if (dhi - dlo + p->ref_len > kRescueMaxRows)
        throw Error(DRM_ERR_UNSUPPORTED, "template lengths [" + std::to_string(p->min_tlen) + ", " +
                                             std::to_string(p->max_tlen) + "] at ref_len " +
                                             std::to_string(p->ref_len) + " give a rescue region of " +
                                             std::to_string(dhi - dlo + p->ref_len) + " > 2048 rows");
}

void drm::check_scoring(const drm_sw_scoring *sc)
{
    auto range = [](const char *name, int32_t v, int32_t lo, int32_t hi) {
        if (v < lo || v > hi)
            throw Error(DRM_ERR_ARG, std::string("scoring: ") + name + " " + std::to_string(v) + " outside [" +
                                         std::to_string(lo) + ", " + std::to_string(hi) + "]");
    };
    range("match", sc->match, 1, 31);
    range("mismatch", sc->mismatch, 1, 63);
    range("gap_open", sc->gap_open, 0, 63);
    range("gap_extend", sc->gap_extend, 1, 63);
}

void drm::check_align_flank(const char *what, int32_t ref_len, int32_t flank, bool genome)
{
    if (flank < 0)
        throw Error(DRM_ERR_ARG, "negative flank");
    if (flank > 0 && !genome)
        throw Error(DRM_ERR_ARG, "a flank needs a genome handle: a window table holds nothing beside its rows");
    if ((int64_t)ref_len + 2 * (int64_t)flank > kAlignMaxLen)
        throw Error(DRM_ERR_UNSUPPORTED,
                    what ? "window length " + std::to_string(ref_len) + " + 2 * flank " + std::to_string(flank) +
                               " > 256 is not supported by the GPU " + what + " kernel"
                         : std::string("window length + 2 * flank > 256"));
}

void drm::check_align_launch(const char *what, int32_t ref_len, int32_t flank, int max_qlen)
{
    const std::string tail = std::string(" > 256 is not supported by the GPU ") + what + " kernel";
    if (max_qlen > kAlignMaxLen)
        throw Error(DRM_ERR_UNSUPPORTED, "query length " + std::to_string(max_qlen) + tail);
    const int64_t region = (int64_t)ref_len + 2 * (int64_t)flank;
    if (region > kAlignMaxLen) // a kernel without a flank names its window alone
        throw Error(DRM_ERR_UNSUPPORTED,
                    "window length " + std::to_string(ref_len) +
                        (flank ? " + 2 * flank " + std::to_string(flank) + " = " + std::to_string(region) : "") + tail);
}

static uint64_t rescue_window(const drm_rescue_result &r, int32_t ref_len, int64_t glen)
{
    using drm::Error;
    if (r.status != 0)
        throw Error(DRM_ERR_ARG, "the rescue record holds no hit (status " + std::to_string(r.status) + ")");
    if (ref_len < 1 || glen < ref_len)
        throw Error(DRM_ERR_ARG, "ref_len " + std::to_string(ref_len) + " and genome length " + std::to_string(glen) +
                                     " leave no window");
    if (r.region_len < 1 || r.ref_end < 1 || r.ref_end > r.region_len || r.region_start < 0 ||
        r.region_start > glen - r.region_len)
        throw Error(DRM_ERR_ARG, "the rescue record's region or end row does not lie in a genome of " +
                                     std::to_string(glen) + " bases");
    int64_t p =r.reverse ? r.region_start + r.region_len - r.ref_end : r.region_start + r.ref_end - ref_len;
    p = std::min(std::max<int64_t>(p, 0), glen - ref_len);
    return 2 * (uint64_t)p + (r.reverse ? 1u : 0u);
}

static void pair_rescue_choose(const drm_pair_result &pair, int32_t s1, int32_t s2, uint64_t anchor1, uint64_t anchor2,
                               const drm_rescue_result *rA, const drm_rescue_result *rB, int32_t ref_len, int64_t glen,
                               int32_t penalty, int32_t min_score, drm_pair_result &out, uint64_t &rescued_id)
{
    using drm::Error;
    if (pair.status < 0 || pair.status > 4)
        throw Error(DRM_ERR_ARG, "pair status " + std::to_string(pair.status) + " outside [0, 4]");
    out = pair;
    rescued_id = 0;
    const bool validA = rA && rA->status == 0 && rA->score >= min_score;
    const bool validB = rB && rB->status == 0 && rB->score >= min_score;
    const int64_t sumA = validA ? (int64_t)s1 + rA->score : 0, sumB = validB ? (int64_t)rB->score + s2 : 0;
    bool useA = false, useB = false;
    if (pair.status == 1) {
        const int64_t need = (int64_t)s1 + s2 - penalty;
        const bool qa = validA && sumA >= need, qb = validB && sumB >= need;
        useA = qa && (!qb || sumA >= sumB);
        useB = qb && !useA;
    } else if (pair.status == 2) {
        useA = validA;
    } else if (pair.status == 3) {
        useB = validB;
    }
    if (!useA && !useB)
        return;
    const drm_rescue_result &r = useA ? *rA : *rB;
    const uint64_t anchor = useA ? anchor1 : anchor2;
    const uint64_t wr = rescue_window(r, ref_len, glen);
    // the rescued hit lies on the strand opposite to the anchor's: the forward one of the two is f
    const int64_t pa = (int64_t)(anchor >> 1), pr = (int64_t)(wr >> 1);
    const int64_t tlen = (anchor & 1u) ? pa + ref_len - pr : pr + ref_len - pa;
    out.status = useA ? 5 : 6;
    (useA ? out.j2 : out.j1) = -1;
    out.score = (int32_t)(useA ? sumA : sumB);
    out.tlen = (int32_t)tlen;
    rescued_id = wr;
}

extern "C" int drm_mate_rescue_region(const drm_pair_params *p, int64_t glen, uint64_t anchor_id, int64_t *start,
                                      int32_t *len, int32_t *reverse)
{
    return drm::guarded([&] {
        if (!p || !start || !len || !reverse)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        if (glen < 0)
            throw drm::Error(DRM_ERR_ARG, "negative genome length");
        int64_t dlo = 0, dhi = 0;
        drm::check_rescue_params(p, dlo, dhi);
        const drm::GenomeRegion r = drm::rescue_region(anchor_id, glen, p->ref_len, dlo, dhi);
        *start = r.start;
        *len = r.len;
        *reverse = r.reverse;
    });
}

extern "C" int drm_mate_rescue_window(const drm_rescue_result *r, int32_t ref_len, int64_t glen, uint64_t *window_id)
{
    return drm::guarded([&] {
        if (!r || !window_id)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        *window_id = rescue_window(*r, ref_len, glen);
    });
}

extern "C" int drm_pair_rescue_choose(const drm_pair_result *pair, int32_t s1, int32_t s2, uint64_t anchor1,
                                      uint64_t anchor2, const drm_rescue_result *rA, const drm_rescue_result *rB,
                                      int32_t ref_len, int64_t glen, int32_t unpaired_penalty, int32_t min_score,
                                      drm_pair_result *out, uint64_t *rescued_id)
{
    return drm::guarded([&] {
        if (!pair || !out || !rescued_id)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        drm_pair_result o{};
        uint64_t w = 0;
        pair_rescue_choose(*pair, s1, s2, anchor1, anchor2, rA, rB, ref_len, glen, unpaired_penalty, min_score, o, w);
        *out = o;
        *rescued_id = w;
    });
}

// ----------------------------------------------------------------------- mapping quality: the host-only parts
void drm::check_mapq_params(const drm_mapq_params *p)
{
    if (!p)
        throw Error(DRM_ERR_ARG, "null MAPQ parameters");
    if (p->ref_len < 1 || p->ref_len > (1 << 20))
        throw Error(DRM_ERR_ARG, "ref_len " + std::to_string(p->ref_len) + " outside [1, 2^20]");
    if (p->locus_span < 1 || p->locus_span > (1 << 20))
        throw Error(DRM_ERR_ARG, "locus_span " + std::to_string(p->locus_span) + " outside [1, 2^20]");
    if (p->min_score < 0 || p->min_score > (1 << 20))
        throw Error(DRM_ERR_ARG, "min_score " + std::to_string(p->min_score) + " outside [0, 2^20]");
    if (p->sub_band < 0 || p->sub_band > (1 << 20))
        throw Error(DRM_ERR_ARG, "sub_band " + std::to_string(p->sub_band) + " outside [0, 2^20]");
}

static int32_t mapq_value_checked(int64_t s1, int64_t sub, int64_t n_sub, int64_t full, int64_t min_score)
{
    using drm::Error;
    constexpr int64_t lim = (int64_t)1 << 20;
    if (n_sub < 0 || n_sub > lim)
        throw Error(DRM_ERR_ARG, "n_sub " + std::to_string(n_sub) + " outside [0, 2^20]");
    if (min_score < 0 || min_score > lim)
        throw Error(DRM_ERR_ARG, "min_score " + std::to_string(min_score) + " outside [0, 2^20]");
    if (s1 < -lim || s1 > lim || sub < -lim || sub > lim || full < -lim || full > lim)
        throw Error(DRM_ERR_ARG, "s1, sub and full must lie in [-2^20, 2^20]");
    return drm::mapq_value(s1, sub, n_sub, full, min_score);
}

extern "C" int drm_mapq_value(int64_t s1, int64_t sub, int64_t n_sub, int64_t full, int64_t min_score, int32_t *mapq)
{
    return drm::guarded([&] {
        if (!mapq)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        *mapq = mapq_value_checked(s1, sub, n_sub, full, min_score);
    });
}

extern "C" int drm_pair_mapq_rescued(const drm_mapq_params *mp, const drm_pair_result *pairs,
                                     const int32_t *rescue_score, const int32_t *full1, const int32_t *full2,
                                     int64_t npairs, int64_t row_step, drm_pair_mapq_result *inout)
{
    return drm::guarded([&] {
        using drm::Error;
        drm::check_mapq_params(mp);
        if (npairs < 0 || row_step < 1)
            throw Error(DRM_ERR_ARG, "npairs must be >= 0 and row_step >= 1");
        if (npairs > 0 && (!pairs || !rescue_score || !full1 || !full2 || !inout))
            throw Error(DRM_ERR_ARG, "null argument");
        // everything is checked before anything is written
        std::vector<int32_t> q((size_t)npairs, 0);
        for (int64_t p = 0; p < npairs; ++p) {
            const int32_t st = pairs[p].status;
            if (st < 0 || st > 6)
                throw Error(DRM_ERR_ARG, "pair " + std::to_string(p) + ": status " + std::to_string(st) +
                                             " outside [0, 6]");
            if (st == 5 || st == 6)
                q[(size_t)p] = mapq_value_checked(rescue_score[p], 0, 0, (st == 5 ? full2 : full1)[p * row_step],
                                                  mp->min_score);
        }
        for (int64_t p = 0; p < npairs; ++p) {
            if (pairs[p].status == 5)
                inout[p].mapq2 = std::min(inout[p].mapq1, q[(size_t)p]);
            else if (pairs[p].status == 6)
                inout[p].mapq1 = std::min(inout[p].mapq2, q[(size_t)p]);
        }
    });
}

// ----------------------------------------------------------------------- template-length window: the estimator
// (include/drm_hip.h, drm_tlen_estimate). Integers throughout: n < 2^48 (2^16 bins of 32-bit counts), S1 < 2^64,
// S2 < 2^80 and x * S2 < 2^127, so the sums are 128-bit.
using u128 = unsigned __int128;
using i128 = __int128;

static u128 isqrt128(u128 v) // floor(sqrt(v)), one binary digit at a time
{
    u128 r = 0, bit = (u128)1 << 126;
    while (bit > v)
        bit >>= 2;
    for (; bit; bit >>= 2) {
        if (v >= r + bit) {
            v -= r + bit;
            r = (r >> 1) + bit;
        } else {
            r >>= 1;
        }
    }
    return r;
}

static drm_tlen_estimate_t tlen_estimate(const uint32_t *h, int32_t nbins, int32_t min_samples)
{
    drm_tlen_estimate_t e{};
    int64_t n = 0;
    for (int32_t t = 1; t < nbins; ++t)
        n += h[t];
    if (n < min_samples) {
        e.status = 1;
        return e;
    }
    e.n = n;
    // the quartiles: a[idx] is the first T whose running count passes idx
    const int64_t idx[3] = {std::min(n - 1, n / 4), std::min(n - 1, 2 * n / 4), std::min(n - 1, 3 * n / 4)};
    int32_t q[3] = {0, 0, 0};
    int64_t cum = 0;
    for (int32_t t = 1, j = 0; t < nbins && j < 3; ++t) {
        cum += h[t];
        while (j < 3 && cum > idx[j])
            q[j++] = t;
    }
    e.p25 = q[0];
    e.p50 = q[1];
    e.p75 = q[2];
    const int32_t iqr = e.p75 - e.p25;
    e.trim_lo = std::max(1, e.p25 - 2 * iqr);
    e.trim_hi = std::min(nbins - 1, e.p75 + 2 * iqr);
    u128 s1 = 0, s2 = 0;
    int64_t x = 0;
    for (int32_t t = e.trim_lo; t <= e.trim_hi; ++t) {
        x += h[t];
        s1 += (u128)h[t] * (u128)t;
        s2 += (u128)h[t] * (u128)t * (u128)t;
    }
    e.n_trim = x;
    const u128 ux = (u128)x, r = isqrt128(ux * s2 - s1 * s1);
    e.mean = (int32_t)((2 * s1 + ux) / (2 * ux));
    e.sd = (int32_t)((2 * r + ux) / (2 * ux));
    const i128 lo_num = (i128)s1 - 4 * (i128)r;
    i128 lo = lo_num / (i128)x;
    if (lo_num % (i128)x < 0) // floor, not truncation
        --lo;
    const i128 hi = (i128)((s1 + 4 * r + ux - 1) / ux);
    e.low = (int32_t)std::max<i128>(1, std::min<i128>(e.p25 - 3 * iqr, lo));
    e.high = (int32_t)std::max<i128>(e.p75 + 3 * iqr, hi);
    return e;
}

extern "C" int drm_tlen_estimate(const uint32_t *hist_row, int32_t nbins, int32_t min_samples,
                                 drm_tlen_estimate_t *out)
{
    return drm::guarded([&] {
        if (!hist_row || !out)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        if (nbins < 2 || nbins > (1 << 16) + 1)
            throw drm::Error(DRM_ERR_ARG, "nbins " + std::to_string(nbins) + " outside [2, 2^16 + 1]");
        if (min_samples < 1)
            throw drm::Error(DRM_ERR_ARG, "min_samples " + std::to_string(min_samples) + " must be >= 1");
        *out = tlen_estimate(hist_row, nbins, min_samples);
    });
}

// ----------------------------------------------------------------------- duplicate marking: the host-only parts
extern "C" int drm_sam_end5(const drm_sw_alignment *a, int32_t tag_prefix, int64_t region_start, int32_t region_len,
                            int32_t reverse, int64_t *end5)
{
    using drm::Error;
    return drm::guarded([&] {
        if (!a || !end5)
            throw Error(DRM_ERR_ARG, "null argument");
        if (a->status != 0)
            throw Error(DRM_ERR_ARG, "the record holds no complete alignment (status " + std::to_string(a->status) + ")");
        const int64_t lead = (int64_t)a->q_begin - tag_prefix;
        if (tag_prefix < 0 || lead < 0)
            throw Error(DRM_ERR_ARG, "the alignment reaches into the query's prefix tag");
        *end5 = reverse ? region_start + region_len - 1 - a->ref_begin + lead : region_start + a->ref_begin - lead;
    });
}

extern "C" int drm_dup_end_word(int64_t end5, int32_t reverse, uint64_t *word)
{
    using drm::Error;
    return drm::guarded([&] {
        if (!word)
            throw Error(DRM_ERR_ARG, "null argument");
        if (end5 < -((int64_t)1 << 20) || end5 >= ((int64_t)1 << 61))
            throw Error(DRM_ERR_ARG, "end5 " + std::to_string(end5) + " outside [-2^20, 2^61)");
        *word = ((((uint64_t)(end5 + ((int64_t)1 << 20))) << 1) | (reverse != 0 ? 1u : 0u)) + 1;
    });
}

extern "C" int drm_dup_slot(uint64_t lo, uint64_t hi, int64_t slots, int64_t *slot)
{
    using drm::Error;
    return drm::guarded([&] {
        if (!slot)
            throw Error(DRM_ERR_ARG, "null argument");
        if (slots < 1 || slots > ((int64_t)1 << 32) || (slots & (slots - 1)) != 0)
            throw Error(DRM_ERR_ARG, "slots " + std::to_string(slots) + " is no power of two in [1, 2^32]");
        *slot = (int64_t)(drm::dup_hash(lo, hi) & (uint64_t)(slots - 1));
    });
}
