// tools/pipeline.cpp -- MI355X drop-in for the reference `pipeline` executable (src/main.cpp).
//
// Same argv contract (src/main.cpp:12-22):
//   pipeline <index_prefix> <query_seqs.fastq|.fq|.txt|.npy> <ref_seqs.fasta> [EF] [K] [K_clusters]
//            [output_dir] [use_dynamic] [use_streaming]
// Same files: <prefix>/<basename(prefix)>.index + <prefix>/config.txt in (:34-47), and
// <output_dir>/indices.npy (<u8) + distances.npy (<f4) out (:371-384), written from the raw
// HNSW results exactly like save_results. The north-star tail (SW rerank, the commented-out
// post_process_sw_static call at :333-341) runs on the GPU when query sequences are available and
// adds sw_scores.npy (<i4) and sw_ids.npy (<u8) [n, k] (rows of a query with no candidate: -1 / 2^64-1).
// use_dynamic cuts the candidate windows from the genome string on the device (post_process_sw_dynamic
// instead of the static window table); use_streaming writes <output_dir>/results.sam block by block
// (write_sam_streaming) and, like the reference, skips the .npy outputs -- the reference streams only in
// its dynamic branch, so static + streaming writes no result file there either. DRM_SAM_CIGAR=1 replaces the
// reference's pseudo POS / CIGAR in that SAM by the GPU alignment of every row (drm_sw_align); with
// DRM_SAM_SCORING=match,mismatch,open,extend and / or DRM_SAM_FLANK=n beside it, by the affine-gap alignment over the
// window widened by n genome bases on either side (drm_sw_align_affine).
// DRM_MATES=<fastq of second mates> (with use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1) maps read pairs: the two files
// are interleaved, searched and reranked as one batch, drm_pair_hits chooses one hit per mate (DRM_PAIR_TLEN=min,max,
// DRM_PAIR_PENALTY=n), only those are aligned, and the SAM carries two lines per pair with the pair flags, RNEXT,
// PNEXT and TLEN (drm_sam_pair_fields). DRM_PAIR_RESCUE=1 beside it rescues the mates the search lost: a pair without a
// proper combination has each read aligned against the insert window of its mate's hit (drm_mate_rescue), and a
// rescued mate that scores at least DRM_PAIR_RESCUE_MIN=n replaces the unpaired choice (drm_pair_rescue_choose).
// DRM_SAM_MAPQ=1 (with use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1, one device) replaces the constant MAPQ 60 by the
// locus scan of each read's rerank rows (drm_hit_mapq; for pairs drm_pair_mapq and drm_pair_mapq_rescued), with
// DRM_MAPQ_MIN=n and DRM_MAPQ_SPAN=n; the SW rerank then runs whatever the stride, as with DRM_MATES.
// Sequence inputs are embedded by the reference's GRU model on the GPU (drm_vectorize) when
// DRM_ENCODER names it (.xml IR or .drmenc) or when the reference's models/ path exists in the working
// directory (Config::Inference::MODEL_PATH); otherwise by the deterministic 3-mer stand-in. The rerank is
// the north star's SW rerank (the reference's main runs an L2 rerank with the model at this point,
// src/main.cpp:312-331).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <iostream>
#include <memory>
#include <numeric>
#include <thread>

#include "drm_hip.h"
#include "drm_internal.h"

using clk = std::chrono::high_resolution_clock;
static long ms_since(clk::time_point t0)
{
    return (long)std::chrono::duration_cast<std::chrono::milliseconds>(clk::now() - t0).count();
}

static void check(int rc)
{
    if (rc != DRM_OK)
        throw drm::Error(rc, drm_last_error());
}

// pinned host buffer (drm_host_alloc): the executor's copies become DMA transfers beside the kernels
template <class T> struct Pinned {
    T *p = nullptr;
    explicit Pinned(size_t n)
    {
        void *v = nullptr;
        check(drm_host_alloc(&v, sizeof(T) * std::max<size_t>(n, 1)));
        p = static_cast<T *>(v);
    }
    ~Pinned() { drm_host_free(p); }
    Pinned(const Pinned &) = delete;
    Pinned &operator=(const Pinned &) = delete;
};

// DRM_SAM_CIGAR=1: the GPU alignments (drm_sw_align) of one SAM block's rows, ids[i * k + j] for j < cnt[i] against
// query lo + i. The first pass keeps 16 operation words per row; the rows that need more (status 2) are aligned
// again as a sub-list with a stride that cannot overflow. Rows past cnt[i] keep an empty record. With `affine` the
// rows are aligned by drm_sw_align_affine over their flanked regions, which are kept for the formatter.
struct AffineMode {
    drm_sw_scoring scoring;
    int32_t flank;
};
struct BlockAlignments {
    std::vector<drm_sw_alignment> rec;
    std::vector<uint32_t> ops;
    std::vector<int64_t> off, region_start;
    std::vector<int32_t> region_len;
    drm::SamAlignments view() const
    {
        drm::SamAlignments v{rec.data(), ops.data(), off.data()};
        if (!region_start.empty()) {
            v.region_start = region_start.data();
            v.region_len = region_len.data();
        }
        return v;
    }

    void align(drm_refs *rt, const uint64_t *ids, const int32_t *cnt, size_t m, size_t k, const uint8_t *queries,
               const int32_t *q_len, int32_t q_stride, int32_t ref_len, const AffineMode *affine)
    {
        auto run = [&](const uint64_t *w, const int64_t *q, size_t n, drm_sw_alignment *r, uint32_t *o, int32_t stride) {
            return affine ? drm_sw_align_affine(rt, &affine->scoring, affine->flank, w, q, (int64_t)n, queries, q_len,
                                                q_stride, (int64_t)m, r, o, stride)
                          : drm_sw_align(rt, w, q, (int64_t)n, queries, q_len, q_stride, (int64_t)m, r, o, stride);
        };
        constexpr int32_t kStride = 16;
        constexpr size_t kChunk = (size_t)1 << 20; // pairs per launch
        std::vector<uint64_t> wid;
        std::vector<int64_t> pq, row;
        for (size_t i = 0; i < m; ++i)
            for (size_t j = 0; j < k && (int64_t)j < (int64_t)cnt[i]; ++j) {
                wid.push_back(ids[i * k + j]);
                pq.push_back((int64_t)i);
                row.push_back((int64_t)(i * k + j));
            }
        const size_t np = wid.size();
        rec.assign(m * k, drm_sw_alignment{0, 0, 0, 0, 0, 0, 0, 1});
        off.assign(m * k, 0);
        std::vector<drm_sw_alignment> r1(np);
        std::vector<uint32_t> o1(np * kStride);
        for (size_t c = 0; c < np; c += kChunk) {
            const size_t nc = std::min(kChunk, np - c);
            check(run(wid.data() + c, pq.data() + c, nc, r1.data() + c, o1.data() + c * kStride, kStride));
        }
        std::vector<uint64_t> wid2;
        std::vector<int64_t> pq2, idx2;
        for (size_t p = 0; p < np; ++p)
            if (r1[p].status == 2) {
                wid2.push_back(wid[p]);
                pq2.push_back(pq[p]);
                idx2.push_back((int64_t)p);
            }
        const int32_t full = q_stride + ref_len + (affine ? 2 * affine->flank : 0);
        std::vector<drm_sw_alignment> r2(wid2.size());
        std::vector<uint32_t> o2(wid2.size() * (size_t)full);
        for (size_t c = 0; c < wid2.size(); c += kChunk) {
            const size_t nc = std::min(kChunk, wid2.size() - c);
            check(run(wid2.data() + c, pq2.data() + c, nc, r2.data() + c, o2.data() + c * (size_t)full, full));
        }
        ops.clear();
        size_t x2 = 0;
        for (size_t p = 0; p < np; ++p) {
            const bool retried = x2 < idx2.size() && idx2[x2] == (int64_t)p;
            const drm_sw_alignment &r = retried ? r2[x2] : r1[p];
            const uint32_t *o = retried ? o2.data() + x2 * (size_t)full : o1.data() + p * kStride;
            x2 += retried;
            rec[(size_t)row[p]] = r;
            off[(size_t)row[p]] = (int64_t)ops.size();
            ops.insert(ops.end(), o, o + r.n_ops);
        }
        if (affine) {
            region_start.assign(m * k, 0);
            region_len.assign(m * k, 0);
            for (size_t p = 0; p < np; ++p) {
                int32_t rev = 0;
                check(drm_sw_align_region(rt, wid[p], affine->flank, &region_start[(size_t)row[p]],
                                          &region_len[(size_t)row[p]], &rev));
            }
        }
    }
};

// DRM_SAM_SCORING=match,mismatch,open,extend and DRM_SAM_FLANK=n (with DRM_SAM_CIGAR=1 only): strictly parsed, and
// checked against drm_sw_align_affine's ranges before any work. A flank alone means the scoring 1,1,0,1.
static bool parse_int(const std::string &t, long &v)
{
    if (t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos)
        return false;
    v = std::stol(t);
    return true;
}

static bool affine_mode_from_env(size_t ref_len, AffineMode &mode)
{
    const char *sc = std::getenv("DRM_SAM_SCORING"), *fl = std::getenv("DRM_SAM_FLANK");
    if (!sc && !fl)
        return false;
    mode = AffineMode{{1, 1, 0, 1}, 0};
    if (sc) {
        std::vector<long> v;
        const std::string s(sc);
        for (size_t p = 0; p <= s.size();) {
            size_t q = s.find(',', p);
            if (q == std::string::npos)
                q = s.size();
            long x = 0;
            if (!parse_int(s.substr(p, q - p), x))
                throw drm::Error(DRM_ERR_ARG, "DRM_SAM_SCORING must be match,mismatch,open,extend (four non-negative "
                                              "integers): \"" + s + "\"");
            v.push_back(x);
            p = q + 1;
        }
        if (v.size() != 4 || v[0] < 1 || v[0] > 31 || v[1] < 1 || v[1] > 63 || v[2] > 63 || v[3] < 1 || v[3] > 63)
            throw drm::Error(DRM_ERR_ARG, "DRM_SAM_SCORING must be match,mismatch,open,extend with match 1..31, "
                                          "mismatch 1..63, open 0..63, extend 1..63: \"" + s + "\"");
        mode.scoring = drm_sw_scoring{(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3]};
    }
    if (fl) {
        long x = 0;
        if (!parse_int(fl, x))
            throw drm::Error(DRM_ERR_ARG, std::string("DRM_SAM_FLANK must be a non-negative integer: \"") + fl + "\"");
        if (ref_len + 2 * (size_t)x > 256)
            throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_SAM_FLANK " + std::to_string(x) + ": ref_len " +
                                                      std::to_string(ref_len) + " + 2 * flank > 256");
        mode.flank = (int32_t)x;
    }
    return true;
}

// DRM_MATES=<second mates> turns the paired mode on; DRM_PAIR_TLEN=min,max (default 0,1000) and DRM_PAIR_PENALTY=n
// (default 17, bwa-mem's unpaired penalty) are read only then, as strictly as DRM_SAM_SCORING, and checked against
// drm_pair_hits' ranges before any work. DRM_PAIR_RESCUE=1 turns the mate rescue on; only then is DRM_PAIR_RESCUE_MIN=n
// (0 to 2^20, the score a rescued mate needs) read, as strictly, and the template-length window checked against
// drm_mate_rescue's 2,048-row cap.
constexpr int32_t kRescueMinDefault = 49; // the largest chance score measured, 39, plus 10
struct PairMode {
    std::string mates;
    drm_pair_params prm;
    bool rescue = false;
    int32_t rescue_min = kRescueMinDefault;
};

static bool pair_mode_from_env(size_t ref_len, PairMode &mode)
{
    const char *mates = std::getenv("DRM_MATES");
    if (!mates)
        return false;
    if (!*mates)
        throw drm::Error(DRM_ERR_ARG, "DRM_MATES is empty: it names the file of second mates");
    if (ref_len < 1 || ref_len > ((size_t)1 << 20))
        throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_MATES: ref_len " + std::to_string(ref_len) + " outside [1, 2^20]");
    mode.mates = mates;
    mode.prm = drm_pair_params{(int32_t)ref_len, 0, 1000, 17};
    if (const char *tl = std::getenv("DRM_PAIR_TLEN")) {
        const std::string s(tl);
        const size_t c = s.find(',');
        long lo = 0, hi = 0;
        if (c == std::string::npos || !parse_int(s.substr(0, c), lo) || !parse_int(s.substr(c + 1), hi))
            throw drm::Error(DRM_ERR_ARG, "DRM_PAIR_TLEN must be min,max (two non-negative integers): \"" + s + "\"");
        if (lo > hi || hi > (1L << 30))
            throw drm::Error(DRM_ERR_ARG, "DRM_PAIR_TLEN must be min,max with 0 <= min <= max <= 2^30: \"" + s + "\"");
        mode.prm.min_tlen = (int32_t)lo;
        mode.prm.max_tlen = (int32_t)hi;
    }
    if (const char *pe = std::getenv("DRM_PAIR_PENALTY")) {
        long x = 0;
        if (!parse_int(pe, x) || x > (1L << 20))
            throw drm::Error(DRM_ERR_ARG, std::string("DRM_PAIR_PENALTY must be an integer in [0, 2^20]: \"") + pe + "\"");
        mode.prm.unpaired_penalty = (int32_t)x;
    }
    mode.rescue = std::getenv("DRM_PAIR_RESCUE") && std::atoi(std::getenv("DRM_PAIR_RESCUE")) != 0;
    if (mode.rescue) {
        if (const char *mi = std::getenv("DRM_PAIR_RESCUE_MIN")) {
            long x = 0;
            if (!parse_int(mi, x) || x > (1L << 20))
                throw drm::Error(DRM_ERR_ARG,
                                 std::string("DRM_PAIR_RESCUE_MIN must be an integer in [0, 2^20]: \"") + mi + "\"");
            mode.rescue_min = (int32_t)x;
        }
        int64_t dlo = 0, dhi = 0;
        drm::check_rescue_params(&mode.prm, dlo, dhi); // DRM_PAIR_TLEN wider than the rescue's 2,048 rows
    }
    return true;
}

// DRM_SAM_MAPQ=1 (with use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1 only): the MAPQ column comes from the locus scan of
// each read's rerank rows (drm_hit_mapq, drm_pair_mapq) instead of the constant 60. DRM_MAPQ_MIN=n (default 39, the
// largest chance score DESIGN.md sec. 4.11 recorded for 150-base reads) and DRM_MAPQ_SPAN=n (default ref_len) are read
// only then, as strictly as DRM_SAM_SCORING; sub_band is 2, one substitution under the rerank's scoring {1, 1, 0, 1}.
constexpr int32_t kMapqMinDefault = 39;
static bool mapq_mode_from_env(size_t ref_len, drm_mapq_params &prm)
{
    const char *on = std::getenv("DRM_SAM_MAPQ");
    if (!on || std::atoi(on) == 0)
        return false;
    if (ref_len < 1 || ref_len > ((size_t)1 << 20))
        throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_SAM_MAPQ: ref_len " + std::to_string(ref_len) + " outside [1, 2^20]");
    prm = drm_mapq_params{(int32_t)ref_len, (int32_t)ref_len, kMapqMinDefault, 2};
    if (const char *mi = std::getenv("DRM_MAPQ_MIN")) {
        long x = 0;
        if (!parse_int(mi, x) || x > (1L << 20))
            throw drm::Error(DRM_ERR_ARG, std::string("DRM_MAPQ_MIN must be an integer in [0, 2^20]: \"") + mi + "\"");
        prm.min_score = (int32_t)x;
    }
    if (const char *sp = std::getenv("DRM_MAPQ_SPAN")) {
        long x = 0;
        if (!parse_int(sp, x) || x < 1 || x > (1L << 20))
            throw drm::Error(DRM_ERR_ARG, std::string("DRM_MAPQ_SPAN must be an integer in [1, 2^20]: \"") + sp + "\"");
        prm.locus_span = (int32_t)x;
    }
    if (std::getenv("DRM_SAM_L2_ROWS") && std::atoi(std::getenv("DRM_SAM_L2_ROWS")) != 0)
        throw drm::Error(DRM_ERR_ARG, "DRM_SAM_MAPQ does not go with DRM_SAM_L2_ROWS=1: those rows carry distances, "
                                      "not scores");
    return true;
}

// a read's self score under the rerank's scoring: its length without format_fastq's tags
static int32_t untagged_length(const std::string &tagged)
{
    const int pre = !tagged.empty() && tagged.front() == '<', post = tagged.size() > 1 && tagged.back() == '>';
    return (int32_t)tagged.size() - pre - post;
}

// DRM_PAIR_RESCUE=1, one block of pairs after drm_pair_hits: pair p's reads are the block's queries 2p and 2p + 1, their
// rerank lists ids / scores [2 * npairs][k]. A pair of status 1 gives two tasks (mate 2 against the insert window of
// mate 1's chosen hit, then mate 1 against that of mate 2's), status 2 / 3 one; drm_mate_rescue scores them with the
// rerank's scoring and drm_pair_rescue_choose decides. A rescued mate's window id goes where its chosen row's id
// would be in the list handed to the aligner, and its pair counts as proper. `after` / `rescue_score` (DRM_SAM_MAPQ,
// null otherwise) receive a rescued pair's record and the rescued mate's own score.
static void rescue_block(drm_refs *rt, const PairMode &mode, int64_t glen, const std::vector<drm_pair_result> &res,
                         const uint64_t *ids, const int32_t *scores, size_t k, const uint8_t *queries,
                         const int32_t *q_len, int32_t q_stride, std::vector<uint64_t> &chosen,
                         std::vector<int32_t> &cnt, std::vector<int32_t> &proper,
                         std::vector<drm_pair_result> *after = nullptr, std::vector<int32_t> *rescue_score = nullptr)
{
    const size_t np = res.size();
    auto row_id = [&](size_t read, int32_t j) { return j >= 0 ? ids[read * k + (size_t)j] : (uint64_t)0; };
    auto row_score = [&](size_t read, int32_t j) { return j >= 0 ? scores[read * k + (size_t)j] : 0; };
    std::vector<uint64_t> anchors;
    std::vector<int64_t> tq, slot(2 * np, -1); // slot[2p] = the task anchored on mate 1 (rA), slot[2p + 1] on mate 2
    for (size_t p = 0; p < np; ++p) {
        const int32_t st = res[p].status;
        if (st == 1 || st == 2) {
            slot[2 * p] = (int64_t)anchors.size();
            anchors.push_back(row_id(2 * p, res[p].j1));
            tq.push_back((int64_t)(2 * p + 1));
        }
        if (st == 1 || st == 3) {
            slot[2 * p + 1] = (int64_t)anchors.size();
            anchors.push_back(row_id(2 * p + 1, res[p].j2));
            tq.push_back((int64_t)(2 * p));
        }
    }
    if (anchors.empty())
        return;
    const drm_sw_scoring rerank_scoring{1, 1, 0, 1};
    std::vector<drm_rescue_result> out(anchors.size());
    check(drm_mate_rescue(rt, &rerank_scoring, &mode.prm, anchors.data(), tq.data(), (int64_t)anchors.size(), queries,
                          q_len, q_stride, (int64_t)(2 * np), out.data()));
    for (size_t p = 0; p < np; ++p) {
        if (slot[2 * p] < 0 && slot[2 * p + 1] < 0)
            continue;
        const drm_rescue_result *rA = slot[2 * p] >= 0 ? &out[(size_t)slot[2 * p]] : nullptr;
        const drm_rescue_result *rB = slot[2 * p + 1] >= 0 ? &out[(size_t)slot[2 * p + 1]] : nullptr;
        drm_pair_result r{};
        uint64_t wr = 0;
        check(drm_pair_rescue_choose(&res[p], row_score(2 * p, res[p].j1), row_score(2 * p + 1, res[p].j2),
                                     row_id(2 * p, res[p].j1), row_id(2 * p + 1, res[p].j2), rA, rB, mode.prm.ref_len,
                                     glen, mode.prm.unpaired_penalty, mode.rescue_min, &r, &wr));
        if (r.status != 5 && r.status != 6)
            continue;
        const size_t read = 2 * p + (r.status == 5 ? 1 : 0);
        chosen[read] = wr;
        cnt[read] = 1;
        proper[p] = 1;
        if (after) {
            (*after)[p] = r;
            (*rescue_score)[p] = (r.status == 5 ? rA : rB)->score;
        }
    }
}

int main(int argc, char *argv[])
{
    if (argc < 4 || argc > 10) {
        std::cerr << "Usage: " << argv[0]
                  << " <index_prefix> <query_seqs.fastq> <ref_seqs.fasta> [EF] [K] [K_clusters] [output_dir] "
                     "[use_dynamic] [use_streaming]"
                  << std::endl;
        std::cerr << "  - query input: Can be FASTQ/FASTA/TXT file or pre-computed embeddings in .npy format" << std::endl;
        std::cerr << "  - EF: Optional HNSW search parameter (default: 128)" << std::endl;
        std::cerr << "  - K: Optional number of nearest neighbors to return (default: 128)" << std::endl;
        std::cerr << "  - output_dir: Optional output directory (default: current directory)" << std::endl;
        return 1;
    }
    try {
        auto master = clk::now();
        std::cout << "=== DeepReadMapper MI355X Pipeline ===" << std::endl << std::endl;
        const std::string prefix = argv[1];
        const std::string base = std::filesystem::path(prefix).filename().string();
        const std::string index_file = prefix + "/" + base + ".index";
        const std::string config_file = prefix + "/config.txt";
        if (!std::filesystem::exists(config_file))
            throw drm::Error(DRM_ERR_IO, "Config file does not exist: " + config_file);
        auto config = drm::load_config(config_file);
        if (!config.count("ref_len") || !std::holds_alternative<size_t>(config["ref_len"]) || !config.count("stride") ||
            !std::holds_alternative<size_t>(config["stride"]))
            throw drm::Error(DRM_ERR_FORMAT, "config.txt lacks integer ref_len / stride");
        const size_t ref_len = std::get<size_t>(config["ref_len"]);
        const size_t stride = std::get<size_t>(config["stride"]);
        const std::string query_file = argv[2], ref_file = argv[3];
        const int ef = argc >= 5 ? std::stoi(argv[4]) : 128;
        const int k = argc >= 6 ? std::stoi(argv[5]) : 128;
        int k_clusters = 5;
        if (stride == 1)
            k_clusters = k;
        else if (argc >= 7)
            k_clusters = std::stoi(argv[6]);
        const std::string out_dir = argc >= 8 ? argv[7] : ".";
        const bool use_dynamic = argc >= 9 && std::stoi(argv[8]) != 0;
        const bool use_streaming = argc >= 10 && std::stoi(argv[9]) != 0;
        const std::string sam_file = out_dir + "/results.sam"; // src/main.cpp:67
        AffineMode affine_mode{};
        const bool cigar_env = std::getenv("DRM_SAM_CIGAR") && std::atoi(std::getenv("DRM_SAM_CIGAR")) != 0;
        const AffineMode *affine = cigar_env && affine_mode_from_env(ref_len, affine_mode) ? &affine_mode : nullptr;
        PairMode pair_mode{};
        const bool paired = pair_mode_from_env(ref_len, pair_mode);
        drm_mapq_params mapq_prm{};
        const bool mapq_on = use_dynamic && use_streaming && cigar_env &&
                             std::filesystem::path(argv[2]).extension() != ".npy" && mapq_mode_from_env(ref_len, mapq_prm);
        if (paired) {
            if (!use_dynamic || !use_streaming)
                throw drm::Error(DRM_ERR_ARG, "DRM_MATES needs use_dynamic=1 and use_streaming=1: pairs are written to the "
                                              "streamed SAM");
            if (!cigar_env)
                throw drm::Error(DRM_ERR_ARG, "DRM_MATES needs DRM_SAM_CIGAR=1: the pair fields come from real alignments");
            if (std::filesystem::path(query_file).extension() == ".npy" ||
                std::filesystem::path(pair_mode.mates).extension() == ".npy")
                throw drm::Error(DRM_ERR_ARG, "DRM_MATES needs sequence files for both mates, not .npy embeddings");
        }
        // devices: DRM_DEVICES=0,1,... fans the batch out over several GPUs (contiguous query shards,
        // replicated index); DRM_DEVICE=i picks one (default 0)
        std::vector<int> devices;
        if (const char *dl = std::getenv("DRM_DEVICES")) {
            std::string sdl(dl);
            for (size_t p = 0; p < sdl.size();) {
                size_t q = sdl.find(',', p);
                if (q == std::string::npos)
                    q = sdl.size();
                if (q > p)
                    devices.push_back(std::stoi(sdl.substr(p, q - p)));
                p = q + 1;
            }
        }
        if (devices.empty())
            devices.push_back(std::getenv("DRM_DEVICE") ? std::atoi(std::getenv("DRM_DEVICE")) : 0);
        const int device = devices[0];
        if (paired && devices.size() != 1)
            throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_MATES runs on one device (DRM_DEVICE), not on DRM_DEVICES");
        if (mapq_on && devices.size() != 1)
            throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_SAM_MAPQ runs on one device (DRM_DEVICE), not on DRM_DEVICES");

        // ---- data loading
        std::vector<float> emb;
        size_t nq = 0, dim = 0;
        std::vector<std::string> qseqs, qids;
        const bool is_npy = std::filesystem::path(query_file).extension() == ".npy";
        auto t0 = clk::now();
        if (is_npy) {
            drm::NpyArray a = drm::npy_load(query_file);
            if (a.shape.size() != 2)
                throw drm::Error(DRM_ERR_FORMAT, "Error: Expected 2D array in .npy file");
            if (a.kind != 'f' || a.itemsize != 4)
                throw drm::Error(DRM_ERR_FORMAT, "embeddings .npy must be float32 ('<f4')");
            nq = a.shape[0];
            dim = a.shape[1];
            emb.resize(nq * dim);
            std::memcpy(emb.data(), a.bytes.data(), emb.size() * sizeof(float));
            std::cout << "[MAIN] Loaded " << nq << " embeddings of dimension " << dim << std::endl;
        } else {
            drm::read_file(query_file, qseqs, qids);
            if (qseqs.empty()) {
                std::cerr << "No query_sequences found in input file!" << std::endl;
                return 1;
            }
            if (paired) { // mate 1 of pair i becomes query 2i, mate 2 query 2i + 1
                std::vector<std::string> seqs2, ids2;
                drm::read_file(pair_mode.mates, seqs2, ids2);
                const size_t n1 = qseqs.size(), n2 = seqs2.size();
                auto name = [](const std::vector<std::string> &ids, size_t i) { return i < ids.size() ? ids[i] : std::string(); };
                for (size_t i = 0; i < std::min(n1, n2); ++i)
                    if (name(qids, i) != name(ids2, i))
                        throw drm::Error(DRM_ERR_FORMAT, "DRM_MATES: record " + std::to_string(i) + " is named \"" +
                                                             name(qids, i) + "\" in " + query_file + " and \"" +
                                                             name(ids2, i) + "\" in " + pair_mode.mates);
                if (n1 != n2)
                    throw drm::Error(DRM_ERR_FORMAT, "DRM_MATES: " + query_file + " has " + std::to_string(n1) +
                                                         " records and " + pair_mode.mates + " has " + std::to_string(n2) +
                                                         ": record " + std::to_string(std::min(n1, n2)) + " has no mate");
                std::vector<std::string> seqs(2 * n1), ids(2 * n1);
                for (size_t i = 0; i < n1; ++i) {
                    seqs[2 * i] = std::move(qseqs[i]);
                    seqs[2 * i + 1] = std::move(seqs2[i]);
                    ids[2 * i] = ids[2 * i + 1] = name(qids, i);
                }
                qseqs.swap(seqs);
                qids.swap(ids);
                std::cout << "[MAIN] Paired mode: " << n1 << " pairs, mates from " << pair_mode.mates << std::endl;
            }
            nq = qseqs.size();
        }
        // ---- reference: the static window table (read_file(ref, ref_len, 1, lookup)), or with use_dynamic the
        //      genome string (extract_FASTA_sequence), windows cut on the device (src/main.cpp:182-192)
        const bool dyn = use_dynamic && !is_npy;
        std::vector<std::string> refs;
        std::string genome;
        if (dyn) {
            std::cout << "[MAIN] Using DYNAMIC fetching for reference sequences" << std::endl;
            genome = drm::extract_fasta_sequence(ref_file);
            std::cout << "[MAIN] Loaded a " << genome.size() << " bp genome from " << ref_file << std::endl;
        } else if (!is_npy) {
            std::cout << "[MAIN] Using STATIC fetching for reference sequences" << std::endl;
            std::vector<std::string> dummy;
            drm::read_file(ref_file, refs, dummy, ref_len, 1, true);
            std::cout << "[MAIN] Loaded " << refs.size() << " reference sequences from " << ref_file << std::endl;
            // the device window table is fixed-width: a .txt / .fastq reference whose lines are not
            // all ref_len bytes would be over-read or silently truncated (the reference scores the
            // whole string), so it is refused before anything touches the GPU
            for (size_t r = 0; r < refs.size(); ++r)
                if (refs[r].size() != ref_len)
                    throw drm::Error(DRM_ERR_FORMAT, "reference sequence " + std::to_string(r) + " has " +
                                                         std::to_string(refs[r].size()) +
                                                         " bytes; the window table needs ref_len = " +
                                                         std::to_string(ref_len) + " for every window");
        }
        std::cout << "[MAIN] Total Data loading time: " << ms_since(t0) << " ms" << std::endl << std::endl;

        // ---- window table (static ref_seqs) as one fixed-width block
        std::string table;
        if (!is_npy && !dyn) {
            table.assign(refs.size() * ref_len, '\0');
            for (size_t r = 0; r < refs.size(); ++r)
                std::memcpy(&table[r * ref_len], refs[r].data(), ref_len);
        }

        // ---- index (one replica per device)
        t0 = clk::now();
        if (!std::filesystem::exists(index_file))
            throw drm::Error(DRM_ERR_IO, "Index file does not exist: " + index_file);
        drm_index *index = nullptr;
        drm_refs *rt = nullptr;
        drm_multi *multi = nullptr;
        drm_index_info info;
        if (devices.size() == 1) {
            check(drm_index_load(index_file.c_str(), device, &index));
            check(drm_index_get_info(index, &info));
            if (dyn)
                check(drm_refs_create_genome((const uint8_t *)genome.data(), (int64_t)genome.size(), (int32_t)ref_len,
                                             device, &rt));
            else if (!is_npy)
                check(drm_refs_create((const uint8_t *)table.data(), (int64_t)refs.size(), (int32_t)ref_len,
                                      (int64_t)ref_len, device, &rt));
        } else {
            if (dyn)
                check(drm_multi_create_genome(index_file.c_str(), devices.data(), (int)devices.size(),
                                              (const uint8_t *)genome.data(), (int64_t)genome.size(), (int32_t)ref_len,
                                              &multi));
            else
                check(drm_multi_create(index_file.c_str(), devices.data(), (int)devices.size(),
                                       is_npy ? nullptr : (const uint8_t *)table.data(), (int64_t)refs.size(),
                                       (int32_t)ref_len, (int64_t)ref_len, &multi));
            check(drm_multi_get_index_info(multi, &info));
        }
        if (index) { // the executor's streams and buffers for this batch, outside the search timing
            size_t qs_max = 0;
            for (auto &q : qseqs)
                qs_max = std::max(qs_max, q.size());
            check(drm_search_rerank_prepare(index, (int64_t)nq, (int32_t)(is_npy ? dim : info.d), k_clusters, k,
                                            is_npy ? 0 : (int32_t)qs_max));
        }
        std::cout << "[MAIN] Index loaded time: " << ms_since(t0) << " ms (" << info.ntotal << " vectors, "
                  << info.device_bytes / (1 << 20) << " MiB on each of " << devices.size() << " device(s))"
                  << std::endl;

        // ---- embedding (Vectorizer::vectorize, src/main.cpp:249-268), into pinned host memory: the GRU model
        //      on the GPU (DRM_ENCODER or the reference's models/ path), else the deterministic 3-mer stand-in
        if (!is_npy)
            dim = (size_t)info.d;
        Pinned<float> x(nq * dim);
        if (!is_npy) {
            t0 = clk::now();
            const std::string model = drm::encoder_model_path();
            if (!model.empty()) {
                if (dim != 128)
                    throw drm::Error(DRM_ERR_ARG, "the GRU model emits 128-d embeddings; the index has d = " +
                                                      std::to_string(dim));
                drm::vectorize_host(model, device, qseqs, x.p);
                std::cout << "[MAIN] Inference (GRU model " << model << ", GPU) time: " << ms_since(t0) << " ms"
                          << std::endl;
            } else {
                std::string all;
                std::vector<int64_t> off(nq);
                std::vector<int32_t> len(nq);
                for (size_t i = 0; i < nq; ++i) {
                    off[i] = (int64_t)all.size();
                    len[i] = (int32_t)qseqs[i].size();
                    all += qseqs[i];
                }
                check(drm_embed_kmer3((const uint8_t *)all.data(), off.data(), len.data(), (int64_t)nq, (int32_t)dim,
                                      drm::kEmbedSeed, x.p));
                std::cout << "[MAIN] Inference (3-mer stand-in) time: " << ms_since(t0) << " ms" << std::endl;
            }
        } else {
            std::memcpy(x.p, emb.data(), sizeof(float) * nq * dim);
        }

        // ---- HNSW search (faiss_search(alg_hnsw, embeddings, k_clusters, ef), src/main.cpp:278) streamed into
        //      the SW rerank (post_process_sw_static, :333-341) batch by batch
        size_t qs = 0;
        for (auto &q : qseqs)
            qs = std::max(qs, q.size());
        Pinned<uint8_t> qbuf(nq * std::max<size_t>(qs, 1));
        Pinned<int32_t> ql(nq), status(nq);
        for (size_t i = 0; i < nq && !is_npy; ++i) {
            std::memset(qbuf.p + i * qs, 0, qs);
            std::memcpy(qbuf.p + i * qs, qseqs[i].data(), qseqs[i].size());
            ql.p[i] = (int32_t)qseqs[i].size();
        }
        Pinned<float> D(nq * (size_t)k_clusters);
        Pinned<int64_t> I(nq * (size_t)k_clusters);
        Pinned<int32_t> sw_scores(is_npy ? 0 : nq * (size_t)k);
        Pinned<uint64_t> sw_ids(is_npy ? 0 : nq * (size_t)k);
        t0 = clk::now();
        drm_search_stats st{};
        // The reference streams its SAM from post_process_l2_dynamic_streaming (src/main.cpp:316-319). With a
        // dense index (stride 1) that function skips every reranker and writes the first min(k, k_clusters)
        // search neighbours of each query in search order (src/utils/post_processor.cpp:833-878), so the SAM
        // here comes straight from the search and no rerank runs. A sparse index reranks the expanded windows of
        // the whole run by L2 (:884-1010): drm_post_process_l2_dynamic over every query after the search, on a
        // window-embedding table of the genome built by the GRU model. Without the model (3-mer stand-in) or
        // across several devices, those SAM rows come from the SW rerank instead.
        //
        // What the reference's sparse branch writes is only the SAM header: its write_sam_streaming call there
        // (post_processor.cpp:1004-1005) leaves out batch_query_count, which defaults to 0
        // (includes/utils/utils.hpp:99), so the row loop (utils.cpp:452) never runs. That header-only file is
        // the default here too (no rerank is computed for it). DRM_SAM_L2_ROWS=1 opts into the rows the
        // reranker meant to write: the L2 rows of every query, and none for a query whose
        // candidate range runs past the clipped expansion stream (the reference reads out of bounds there).
        const bool stream_sam = use_streaming && dyn;
        // DRM_MATES, DRM_SAM_MAPQ: pairing and MAPQ need scores, so the SW rerank runs whatever the stride
        const bool sam_from_search = stream_sam && stride == 1 && !paired && !mapq_on;
        const bool l2_rows = std::getenv("DRM_SAM_L2_ROWS") && std::atoi(std::getenv("DRM_SAM_L2_ROWS")) != 0;
        const bool sam_header_only = stream_sam && stride > 1 && !l2_rows && !paired && !mapq_on;
        // DRM_SAM_CIGAR=1: every SAM row gets its real POS / CIGAR / AS / NM from a GPU
        // alignment of the block's rows (drm_sw_align) before the host thread formats the block. Unset: no
        // alignment is launched and the file is the reference's.
        const bool sam_cigar = stream_sam && !sam_header_only && std::getenv("DRM_SAM_CIGAR") &&
                               std::atoi(std::getenv("DRM_SAM_CIGAR")) != 0;
        drm_refs *art = rt; // the handle the alignments run on (several devices: one more genome handle on the first)
        if (sam_cigar && !art)
            check(drm_refs_create_genome((const uint8_t *)genome.data(), (int64_t)genome.size(), (int32_t)ref_len, device,
                                         &art));
        // rows of one alignment pass: DRM_SAM_BLOCK when set, else blocks of about 4M rows
        auto sam_block = [&](size_t rows_per_query) {
            size_t block = 1u << 20;
            if (const char *e = std::getenv("DRM_SAM_BLOCK"))
                block = std::max<size_t>(1, std::strtoull(e, nullptr, 10));
            else if (sam_cigar)
                block = std::max<size_t>(1, std::min<size_t>(block, ((size_t)1 << 22) / std::max<size_t>(rows_per_query, 1)));
            return block;
        };
        const bool sam_l2 = stream_sam && stride > 1 && l2_rows && rt && !is_npy && !drm::encoder_model_path().empty() &&
                            !paired;
        if (stream_sam && (size_t)k > (size_t)k_clusters * 2 * stride) // post_processor.cpp:769-772
            throw drm::Error(DRM_ERR_K, "Final k too large. Ensure k < k_clusters * 2 * stride to have enough candidates.");
        if (stream_sam && stride > 1 && l2_rows && !sam_l2 && !paired)
            std::cout << "[MAIN] stride > 1 without the GRU model on one device: SAM rows from the SW rerank (the "
                         "reference reranks them by L2 here)"
                      << std::endl;
        // one pass over queries [lo, lo + m) into the output arrays at row lo
        auto run = [&](size_t lo, size_t m, drm_search_stats *sp) {
            const bool search_only = sam_from_search || sam_l2 || sam_header_only;
            const uint8_t *qb = (is_npy || search_only) ? nullptr : qbuf.p + lo * qs;
            if (multi)
                return drm_multi_search_rerank(multi, x.p + lo * dim, (int64_t)m, (int32_t)dim, k_clusters, ef, qb,
                                               ql.p + lo, (int32_t)qs, (int64_t)stride, k, D.p + lo * k_clusters,
                                               I.p + lo * k_clusters, sw_scores.p + lo * k, sw_ids.p + lo * k,
                                               status.p + lo, sp);
            return drm_search_rerank(index, search_only ? nullptr : rt, x.p + lo * dim, (int64_t)m,
                                     (int32_t)dim,
                                     k_clusters, ef, qb, ql.p + lo,
                                     (int32_t)qs, (int64_t)stride, k, D.p + lo * k_clusters, I.p + lo * k_clusters,
                                     sw_scores.p + lo * k, sw_ids.p + lo * k, status.p + lo, sp);
        };
        int rc = DRM_OK;
        if (sam_header_only) {
            std::cout << "[MAIN] Using STREAMING output to SAM file: " << sam_file << std::endl;
            std::filesystem::create_directories(out_dir);
            rc = run(0, nq, &st); // faiss_search of the whole run (src/main.cpp:278)
            if (rc == DRM_OK)
                drm::write_sam_block(sam_file, true, "ref", ref_len, qseqs, qids, 0, 0, nullptr, nullptr, (size_t)k);
        } else if (sam_l2) {
            std::cout << "[MAIN] Using STREAMING output to SAM file: " << sam_file << std::endl;
            std::filesystem::create_directories(out_dir);
            rc = run(0, nq, &st);
            if (rc == DRM_OK) {
                const auto tl = clk::now();
                drm_encoder *enc = nullptr;
                check(drm_encoder_load(drm::encoder_model_path().c_str(), device, &enc));
                const int erc = drm_refs_embed(rt, enc, nullptr);
                drm_encoder_free(enc);
                check(erc);
                std::vector<float> l2d(nq * (size_t)k);
                std::vector<uint64_t> l2i(nq * (size_t)k);
                std::vector<int32_t> cnt(nq);
                int64_t bad = -1;
                const int lrc = drm_post_process_l2_dynamic(rt, I.p, (int64_t)nq, k_clusters, x.p, (int32_t)dim,
                                                            (int64_t)stride, k, k_clusters, l2d.data(), l2i.data(),
                                                            cnt.data(), &bad);
                // a candidate range past the clipped stream (status -4): that query keeps no row, the others are
                // written (every output was downloaded before the error was raised)
                if (lrc == DRM_ERR_ARG && bad >= 0) {
                    size_t clipped = 0;
                    for (size_t i = 0; i < nq; ++i)
                        clipped += cnt[i] == 0;
                    std::cout << "[MAIN] " << clipped << " queries (first " << bad
                              << ") rerank past the clipped expansion stream: written without rows" << std::endl;
                } else {
                    check(lrc);
                }
                std::cout << "[MAIN] L2 rerank (dynamic, stride " << stride << ") time: " << ms_since(tl) << " ms"
                          << std::endl;
                const size_t block = sam_block((size_t)k);
                for (size_t lo = 0; lo < nq; lo += block) { // write_sam_streaming per reranked batch (:1004-1006)
                    const size_t m = std::min(block, nq - lo);
                    BlockAlignments ba;
                    drm::SamAlignments av{};
                    if (sam_cigar) {
                        ba.align(art, l2i.data() + lo * k, cnt.data() + lo, m, (size_t)k, qbuf.p + lo * qs, ql.p + lo,
                                 (int32_t)qs, (int32_t)ref_len, affine);
                        av = ba.view();
                    }
                    drm::write_sam_block(sam_file, lo == 0, "ref", ref_len, qseqs, qids, lo, m, l2i.data() + lo * k,
                                         cnt.data() + lo, (size_t)k, sam_cigar ? &av : nullptr);
                }
            }
        } else if (paired) {
            // per block of pairs: search + SW rerank of its 2m interleaved reads, drm_pair_hits over the block's
            // lists (row_step 2), the alignment of only the chosen row of every read, and the two lines per pair from
            // the writer thread while the GPU works on the next block. DRM_SAM_BLOCK counts pairs here; the file does
            // not depend on it.
            std::cout << "[MAIN] Using STREAMING output to SAM file: " << sam_file << " (paired)" << std::endl;
            std::filesystem::create_directories(out_dir);
            const size_t npairs = nq / 2, block = sam_block(2);
            std::thread writer;
            std::string werr;
            for (size_t p0 = 0; p0 < npairs && rc == DRM_OK; p0 += block) {
                const size_t mp = std::min(block, npairs - p0), lo = 2 * p0, m = 2 * mp;
                drm_search_stats bs{};
                rc = run(lo, m, &bs);
                st.nq += bs.nq;
                st.ndis += bs.ndis;
                st.nhops += bs.nhops;
                st.kernel_ms += bs.kernel_ms;
                auto ids = std::make_shared<std::vector<uint64_t>>(m, 0);
                auto cnt = std::make_shared<std::vector<int32_t>>(m, 0);
                auto proper = std::make_shared<std::vector<int32_t>>(mp, 0);
                auto line_mapq = std::make_shared<std::vector<int32_t>>(mapq_on ? m : 0, 0);
                auto ba = std::make_shared<BlockAlignments>();
                if (rc == DRM_OK) {
                    try {
                        std::vector<drm_pair_result> res(mp);
                        check(drm_set_device(device));
                        const size_t at = lo * (size_t)k;
                        check(drm_pair_hits(&pair_mode.prm, sw_ids.p + at, sw_scores.p + at, status.p + lo,
                                            sw_ids.p + at + k, sw_scores.p + at + k, status.p + lo + 1, (int64_t)mp, k, 2,
                                            res.data()));
                        for (size_t p = 0; p < mp; ++p) {
                            const int32_t j[2] = {res[p].j1, res[p].j2};
                            for (size_t t = 0; t < 2; ++t)
                                if (j[t] >= 0) {
                                    (*ids)[2 * p + t] = sw_ids.p[(lo + 2 * p + t) * (size_t)k + (size_t)j[t]];
                                    (*cnt)[2 * p + t] = 1;
                                }
                            (*proper)[p] = res[p].status == 0;
                        }
                        // DRM_SAM_MAPQ: the pair MAPQ of the same lists, before a rescue changes the choice
                        std::vector<drm_pair_mapq_result> pm(mapq_on ? mp : 0);
                        std::vector<int32_t> full(mapq_on ? m : 0), rescue_score(mapq_on ? mp : 0, 0);
                        std::vector<drm_pair_result> after;
                        if (mapq_on) {
                            for (size_t r = 0; r < m; ++r)
                                full[r] = untagged_length(qseqs[lo + r]);
                            check(drm_pair_mapq(&pair_mode.prm, &mapq_prm, sw_ids.p + at, sw_scores.p + at, status.p + lo,
                                                sw_ids.p + at + k, sw_scores.p + at + k, status.p + lo + 1, full.data(),
                                                full.data() + 1, res.data(), (int64_t)mp, k, 2, pm.data()));
                            after = res;
                        }
                        if (pair_mode.rescue)
                            rescue_block(art, pair_mode, (int64_t)genome.size(), res, sw_ids.p + at, sw_scores.p + at,
                                         (size_t)k, qbuf.p + lo * qs, ql.p + lo, (int32_t)qs, *ids, *cnt, *proper,
                                         mapq_on ? &after : nullptr, mapq_on ? &rescue_score : nullptr);
                        if (mapq_on) {
                            if (pair_mode.rescue)
                                check(drm_pair_mapq_rescued(&mapq_prm, after.data(), rescue_score.data(), full.data(),
                                                            full.data() + 1, (int64_t)mp, 2, pm.data()));
                            for (size_t p = 0; p < mp; ++p) {
                                (*line_mapq)[2 * p] = pm[p].mapq1;
                                (*line_mapq)[2 * p + 1] = pm[p].mapq2;
                            }
                        }
                        ba->align(art, ids->data(), cnt->data(), m, 1, qbuf.p + lo * qs, ql.p + lo, (int32_t)qs,
                                  (int32_t)ref_len, affine);
                    } catch (...) {
                        if (writer.joinable())
                            writer.join();
                        throw;
                    }
                }
                if (writer.joinable())
                    writer.join();
                if (rc == DRM_OK && werr.empty())
                    writer = std::thread([&, lo, mp, ids, cnt, proper, ba, line_mapq] {
                        try {
                            drm::write_sam_pairs(sam_file, lo == 0, "ref", ref_len, qseqs, qids, lo, mp, ids->data(),
                                                 cnt->data(), proper->data(), ba->view(),
                                                 mapq_on ? line_mapq->data() : nullptr);
                        } catch (const std::exception &e) {
                            werr = e.what();
                        }
                    });
            }
            if (writer.joinable())
                writer.join();
            if (rc == DRM_OK && !werr.empty())
                throw drm::Error(DRM_ERR_IO, werr);
        } else if (stream_sam) {
            // post_process_*_dynamic_streaming + write_sam_streaming (src/main.cpp:316-319,
            // src/utils/utils.cpp:409-503): the SAM lines of each block are written by a host thread while the
            // GPU works on the next block (blocks of DRM_SAM_BLOCK queries; the file does not depend on it)
            std::cout << "[MAIN] Using STREAMING output to SAM file: " << sam_file << std::endl;
            std::filesystem::create_directories(out_dir);
            const size_t block = sam_block(sam_from_search ? (size_t)std::min(k, k_clusters) : (size_t)k);
            std::thread writer;
            std::string werr;
            for (size_t lo = 0; lo < nq && rc == DRM_OK; lo += block) {
                const size_t m = std::min(block, nq - lo);
                drm_search_stats bs{};
                rc = run(lo, m, &bs);
                st.nq += bs.nq;
                st.ndis += bs.ndis;
                st.nhops += bs.nhops;
                st.kernel_ms += bs.kernel_ms;
                // the block's rows, and with DRM_SAM_CIGAR their alignments: on the GPU from this thread, while
                // the writer still formats the previous block
                const size_t kr = sam_from_search ? (size_t)k_clusters : (size_t)k;
                const uint64_t *rows = sam_from_search ? reinterpret_cast<const uint64_t *>(I.p) + lo * k_clusters
                                                       : sw_ids.p + lo * k;
                auto cnt = std::make_shared<std::vector<int32_t>>(m);
                auto line_mapq = std::make_shared<std::vector<int32_t>>(mapq_on ? m * kr : 0, 0);
                auto ba = std::make_shared<BlockAlignments>();
                if (rc == DRM_OK) {
                    for (size_t i = 0; i < m; ++i)
                        (*cnt)[i] = sam_from_search ? std::min(k, k_clusters) : std::max(status.p[lo + i], 0);
                    if (sam_cigar) {
                        try {
                            if (mapq_on) { // DRM_SAM_MAPQ: the locus scan of the block's rerank rows, head = the primary row
                                std::vector<int32_t> full(m), head(m, 0);
                                std::vector<drm_mapq_result> res(m);
                                for (size_t i = 0; i < m; ++i)
                                    full[i] = untagged_length(qseqs[lo + i]);
                                check(drm_set_device(device));
                                check(drm_hit_mapq(&mapq_prm, rows, sw_scores.p + lo * k, status.p + lo, head.data(),
                                                   full.data(), (int64_t)m, k, res.data()));
                                for (size_t i = 0; i < m; ++i)
                                    (*line_mapq)[i * kr] = res[i].mapq; // secondary lines print 0
                            }
                            ba->align(art, rows, cnt->data(), m, kr, qbuf.p + lo * qs, ql.p + lo, (int32_t)qs,
                                      (int32_t)ref_len, affine);
                        } catch (...) {
                            if (writer.joinable())
                                writer.join();
                            throw;
                        }
                    }
                }
                if (writer.joinable())
                    writer.join();
                if (rc == DRM_OK && werr.empty())
                    writer = std::thread([&, lo, m, kr, rows, cnt, ba, line_mapq] {
                        try {
                            const drm::SamAlignments av = ba->view();
                            drm::write_sam_block(sam_file, lo == 0, "ref", ref_len, qseqs, qids, lo, m, rows,
                                                 cnt->data(), kr, sam_cigar ? &av : nullptr,
                                                 mapq_on ? line_mapq->data() : nullptr);
                        } catch (const std::exception &e) {
                            werr = e.what();
                        }
                    });
            }
            if (writer.joinable())
                writer.join();
            if (rc == DRM_OK && !werr.empty())
                throw drm::Error(DRM_ERR_IO, werr);
        } else {
            rc = run(0, nq, &st);
        }
        const std::string err = rc == DRM_OK ? "" : drm_last_error();
        const long search_ms = ms_since(t0);
        if (art && art != rt)
            drm_refs_free(art);
        if (rt)
            drm_refs_free(rt);
        if (index)
            drm_index_free(index);
        if (multi)
            drm_multi_free(multi);
        if (rc != DRM_OK)
            throw drm::Error(rc, err);
        std::cout << "[MAIN] Search" << (is_npy ? "" : " + SW rerank") << " time: " << search_ms << " ms (device "
                  << st.kernel_ms << " ms, ndis " << st.ndis << ", nhops " << st.nhops << ", " << devices.size()
                  << " device(s))" << std::endl;
        if (!is_npy) // rows of a query with no candidate at all (reranker.cpp:10-11) stay -1 / 2^64-1
            for (size_t i = 0; i < nq; ++i)
                for (int j = std::max(status.p[i], 0); j < k; ++j) {
                    sw_scores.p[i * (size_t)k + (size_t)j] = -1;
                    sw_ids.p[i * (size_t)k + (size_t)j] = ~0ull;
                }

        // ---- outputs (save_results, src/utils/utils.cpp:264-334); skipped with use_streaming (src/main.cpp:371, :409-412)
        if (use_streaming) {
            std::cout << "[MAIN] Skip normal output saving since streaming output is used." << std::endl;
            std::cout << "[MAIN] Total pipeline time: " << ms_since(master) << " ms" << std::endl;
            std::cout << "=== Pipeline Completed Successfully! ===" << std::endl;
            return 0;
        }
        t0 = clk::now();
        std::filesystem::create_directories(out_dir);
        const size_t kout = stride == 1 ? (size_t)k : (size_t)k_clusters;
        std::vector<uint64_t> idx(nq * kout);
        std::vector<float> dis(nq * kout);
        for (size_t i = 0; i < nq; ++i)
            for (size_t j = 0; j < kout; ++j) {
                idx[i * kout + j] = (uint64_t)I.p[i * k_clusters + j];
                dis[i * kout + j] = D.p[i * k_clusters + j];
            }
        drm::npy_save(out_dir + "/indices.npy", idx.data(), {nq, kout}, 'u', 8);
        drm::npy_save(out_dir + "/distances.npy", dis.data(), {nq, kout}, 'f', 4);
        if (!is_npy) {
            drm::npy_save(out_dir + "/sw_scores.npy", sw_scores.p, {nq, (size_t)k}, 'i', 4);
            drm::npy_save(out_dir + "/sw_ids.npy", sw_ids.p, {nq, (size_t)k}, 'u', 8);
        }
        std::cout << "[MAIN] Output saving time: " << ms_since(t0) << " ms" << std::endl;
        std::cout << "[MAIN] Total pipeline time: " << ms_since(master) << " ms" << std::endl;
        std::cout << "=== Pipeline Completed Successfully! ===" << std::endl;
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
