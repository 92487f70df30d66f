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
// window widened by n genome bases on either side (drm_sw_align_affine). DRM_SAM_CLIP=L (1..63; 0 = off) beside
// DRM_SAM_CIGAR=1 makes that alignment end-aware (drm_sw_align_affine_clip, bwa-mem's -L): an alignment that stops short
// of a read end pays L, so a mismatch a few bases from an end is aligned instead of soft-clipped.
// DRM_MATES=<fastq of second mates> (with use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1) maps read pairs: the two files
// are interleaved, searched and reranked as one batch, drm_pair_hits chooses one hit per mate (DRM_PAIR_TLEN=min,max,
// DRM_PAIR_PENALTY=n), only those are aligned, and the SAM carries two lines per pair with the pair flags, RNEXT,
// PNEXT and TLEN (drm_sam_pair_fields). DRM_PAIR_RESCUE=1 beside it rescues the mates the search lost: a pair without a
// proper combination has each read aligned against the insert window of its mate's hit (drm_mate_rescue), and a
// rescued mate that scores at least DRM_PAIR_RESCUE_MIN=n replaces the unpaired choice (drm_pair_rescue_choose).
// DRM_PAIR_TLEN=auto estimates the window from the first DRM_PAIR_TLEN_SAMPLE=n pairs before the block loop: the
// template lengths of the pairs whose mates both reach MAPQ DRM_PAIR_TLEN_MAPQ=n alone (drm_tlen_scan_device), then
// bwa-mem's quartile rule on their histogram (drm_tlen_estimate); the run goes on as with DRM_PAIR_TLEN=<min>,<max>.
// DRM_SAM_MAPQ=1 (with use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1, one device) replaces the constant MAPQ 60 by the
// locus scan of each read's rerank rows (drm_hit_mapq; for pairs drm_pair_mapq and drm_pair_mapq_rescued), with
// DRM_MAPQ_MIN=n and DRM_MAPQ_SPAN=n; the SW rerank then runs whatever the stride, as with DRM_MATES.
// DRM_CONTIGS=1 (with use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1, sequence queries, one device, an index of stride 1
// built with DRM_CONTIGS=1) tells the reference's contigs apart: drm_contig_hits drops every rerank row whose window
// does not lie inside one contig, the pair-level kernels get its spread ids, and the SAM carries one @SQ per contig,
// the contig's name in RNAME and positions that count from the contig's start.
// DRM_SAM_MD=1 (with DRM_SAM_CIGAR=1) appends MD:Z:<string> behind NM:i on every mapped line: a GPU pass over the rows'
// records and operation words (drm_sw_align_md), then drm_sam_md on the writer thread.
// DRM_SAM_LOCI=n (1..64, with DRM_SAM_MAPQ=1 and all it needs) prints one line per distinct locus of a read instead of
// one per rerank row: drm_hit_loci replaces the block's drm_hit_mapq and lists up to n loci that score at least
// DRM_MAPQ_MIN and DRM_LOCI_DROP=pct (default 80) per cent of the primary; only their head rows are aligned; slot 0 is
// the primary line, the others secondary lines (flag 256, MAPQ 0); a read without a locus at or above DRM_MAPQ_MIN is
// written once, unmapped (flag 4). DRM_SAM_XA=1 beside it folds the alternatives into XA:Z:RNAME,<+|->POS,CIGAR,NM;...
// at the end of the primary line. With DRM_MATES the alternatives of every mate whose line comes from a list row are
// aligned in a second pass and appended as XA:Z; nothing else on a paired line changes.
// DRM_SAM_DUP=1 (with DRM_SAM_CIGAR=1 and DRM_MATES or DRM_SAM_LOCI, the modes with one primary placement per read) marks
// duplicate reads and pairs: every block hands the end words of its templates' unclipped 5' ends (drm_sam_end5,
// drm_dup_end_word) to one first-seen set on the device (drm_dupset_mark), and every line of a template whose ends an
// earlier template of the run had carries flag 1024.
// DRM_SAM_SORT=coordinate (with use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1, in every mode those allow; unsorted or
// unset = the file as before, any other value is an error) writes the lines in samtools sort's order under
// @HD SO:coordinate: the writers append every line to a spool in host memory with its key (drm_sam_sort_key of its
// RNAME's @SQ index, POS and strand), and after the last block one stable GPU sort of the keys (drm_sort_order, DESIGN.md
// sec. 4.19) gives the order in which the spool is written; lines of equal key keep the unsorted file's order, so the
// file does not depend on DRM_SAM_BLOCK. The duplicate marks stay first-seen in input order. The spool holds the whole
// run (a few hundred bytes per line); an external merge for runs that do not fit in host memory is not implemented.
// DRM_SAM_STATS=1 prints the SAM stage's time and the rows it aligned, and with DRM_SAM_SORT the sort's and the final
// write's time.
// DRM_SAM_FORMAT=bam (with the same companions as DRM_SAM_SORT; sam or unset = the file as before, any other value is an
// error) writes <output_dir>/results.bam and no results.sam: the BAM header of the same @HD / @SQ text, every line as a BAM
// alignment record in the order the lines would have had (with DRM_SAM_SORT=coordinate the spool holds the records and
// the sorted file is written from them), compressed as BGZF on the GPU (drm_bgzf_compress) in whole
// 65,280-byte blocks with the tail carried across SAM blocks, so the file does not depend on DRM_SAM_BLOCK, and closed
// by the empty EOF member. DRM_SAM_STATS=1 then also prints the bytes in and out of the compression and its time.
// DRM_SAM_QUAL=1 keeps the quality lines of .fastq / .fq queries (and DRM_MATES) and prints them in column 11, reversed
// on a line whose SEQ is reverse-complemented; a quality line of another length than its read ends the run.
// Sequence inputs are embedded by the reference's GRU model on the GPU (drm_vectorize) when
// DRM_ENCODER names it (.xml IR or .drmenc) or when the reference's models/ path exists in the working
// directory (Config::Inference::MODEL_PATH); otherwise by the deterministic 3-mer stand-in. The rerank is
// the north star's SW rerank (the reference's main runs an L2 rerank with the model at this point,
// src/main.cpp:312-331).
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <functional>
#include <iostream>
#include <memory>
#include <numeric>
#include <sstream>
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
    Pinned() = default;
    void alloc(size_t n)
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
// rows are aligned by drm_sw_align_affine over their flanked regions, which are kept for the formatter; with a clipping
// penalty by drm_sw_align_affine_clip, the reads being tagged "<" read ">".
struct AffineMode {
    drm_sw_scoring scoring;
    int32_t flank;
    int32_t clip; // DRM_SAM_CLIP: 0 = the plain affine alignment
};
struct BlockAlignments {
    std::vector<drm_sw_alignment> rec;
    std::vector<uint32_t> ops;
    std::vector<int64_t> off, region_start;
    std::vector<int32_t> region_len;
    // DRM_SAM_MD=1: the MD records and words of the same rows (drm_sw_align_md), by the same two-pass rule
    bool want_md = false;
    std::vector<drm_sw_md> md;
    std::vector<uint32_t> md_words;
    std::vector<int64_t> md_off;
    drm::SamAlignments view() const
    {
        const bool regions = !region_start.empty();
        return {rec.data(), ops.data(), off.data(), regions ? region_start.data() : nullptr,
                regions ? region_len.data() : nullptr, want_md ? md.data() : nullptr,
                want_md ? md_words.data() : nullptr, want_md ? md_off.data() : nullptr};
    }

    // DRM_CONTIGS, the flank guard: row_contig[i * k + j] is the row's contig in `table`. A row keeps its flank iff its
    // region, as drm_sw_align_region clamps it to the genome, lies inside that contig; the others are aligned with flank
    // 0, their window being inside the contig by construction.
    void align(drm_refs *rt, const uint64_t *ids, const int32_t *cnt, size_t m, size_t k, const uint8_t *queries,
               const int32_t *q_len, int32_t q_stride, int32_t ref_len, const AffineMode *affine,
               const drm_contigs *table = nullptr, const int32_t *row_contig = nullptr)
    {
        rec.assign(m * k, drm_sw_alignment{0, 0, 0, 0, 0, 0, 0, 1});
        off.assign(m * k, 0);
        ops.clear();
        if (want_md) {
            md.assign(m * k, drm_sw_md{0, 0, 0, 0, 0, 1});
            md_off.assign(m * k, 0);
            md_words.clear();
        }
        if (affine) {
            region_start.assign(m * k, 0);
            region_len.assign(m * k, 0);
        }
        if (!affine || !table || affine->flank == 0) {
            align_rows(rt, ids, cnt, m, k, queries, q_len, q_stride, ref_len, affine, nullptr);
            return;
        }
        std::vector<uint8_t> inside(m * k, 0);
        for (size_t i = 0; i < m; ++i)
            for (size_t j = 0; j < k && (int64_t)j < (int64_t)cnt[i]; ++j) {
                int64_t start = 0;
                int32_t len = 0, rev = 0, t = -1;
                check(drm_sw_align_region(rt, ids[i * k + j], affine->flank, &start, &len, &rev));
                check(drm_contigs_find(table, start, len, &t));
                inside[i * k + j] = t >= 0 && t == row_contig[i * k + j];
            }
        const AffineMode bare{affine->scoring, 0, affine->clip};
        for (uint8_t &x : inside) // the rows that keep their flank, then the others with none
            x = x ? 1 : 2;
        align_rows(rt, ids, cnt, m, k, queries, q_len, q_stride, ref_len, affine, inside.data(), 1);
        align_rows(rt, ids, cnt, m, k, queries, q_len, q_stride, ref_len, &bare, inside.data(), 2);
    }

    // The two-pass rule of the alignment pass and of the MD pass over a list of np rows. launch(sub, n, stride, records,
    // words) runs the n rows sub[0 .. n) of the list with `stride` words per row. Every row runs at 16 words first, in
    // launches of at most 2^20 rows; the rows that come back with status 2 (more words than that) run again at `full`,
    // the stride that cannot overflow; keep(p, record, words) then sees every row of the list in order, once.
    template <class Rec, class Launch, class Keep>
    static void two_pass(size_t np, int32_t full, Launch &&launch, Keep &&keep)
    {
        constexpr int32_t kStride = 16;
        constexpr size_t kChunk = (size_t)1 << 20; // rows per launch
        auto pass = [&](const std::vector<size_t> &sub, int32_t stride, std::vector<Rec> &r, std::vector<uint32_t> &w) {
            r.resize(sub.size());
            w.resize(sub.size() * (size_t)stride);
            for (size_t c = 0; c < sub.size(); c += kChunk)
                launch(sub.data() + c, std::min(kChunk, sub.size() - c), stride, r.data() + c,
                       w.data() + c * (size_t)stride);
        };
        std::vector<size_t> all(np), again;
        std::iota(all.begin(), all.end(), (size_t)0);
        std::vector<Rec> r1, r2;
        std::vector<uint32_t> w1, w2;
        pass(all, kStride, r1, w1);
        for (size_t p = 0; p < np; ++p)
            if (r1[p].status == 2)
                again.push_back(p);
        pass(again, full, r2, w2);
        for (size_t p = 0, x2 = 0; p < np; ++p) {
            const bool retried = x2 < again.size() && again[x2] == p;
            keep(p, retried ? r2[x2] : r1[p], retried ? w2.data() + x2 * (size_t)full : w1.data() + p * kStride);
            x2 += retried;
        }
    }

    // the rows of the block whose pick[row] == want (pick null: every row), into rec / off / ops / the regions
    void align_rows(drm_refs *rt, const uint64_t *ids, const int32_t *cnt, size_t m, size_t k, const uint8_t *queries,
                    const int32_t *q_len, int32_t q_stride, int32_t ref_len, const AffineMode *affine,
                    const uint8_t *pick, uint8_t want = 0)
    {
        std::vector<uint64_t> wid;
        std::vector<int64_t> pq, row;
        for (size_t i = 0; i < m; ++i)
            for (size_t j = 0; j < k && (int64_t)j < (int64_t)cnt[i]; ++j) {
                if (pick && pick[i * k + j] != want)
                    continue;
                wid.push_back(ids[i * k + j]);
                pq.push_back((int64_t)i);
                row.push_back((int64_t)(i * k + j));
            }
        const size_t np = wid.size();
        const int32_t flank = affine ? affine->flank : 0;
        // the windows and queries of the rows sub[0 .. n), as the aligners take them
        std::vector<uint64_t> w;
        std::vector<int64_t> q;
        auto gather = [&](const size_t *sub, size_t n) {
            w.resize(n);
            q.resize(n);
            for (size_t x = 0; x < n; ++x) {
                w[x] = wid[sub[x]];
                q[x] = pq[sub[x]];
            }
        };
        two_pass<drm_sw_alignment>(
            np, q_stride + ref_len + 2 * flank,
            [&](const size_t *sub, size_t n, int32_t stride, drm_sw_alignment *rc, uint32_t *oc) {
                gather(sub, n);
                const drm_sw_clip clip{affine ? affine->clip : 0, 1, 1};
                check(affine && affine->clip > 0
                          ? drm_sw_align_affine_clip(rt, &affine->scoring, &clip, affine->flank, w.data(), q.data(),
                                                     (int64_t)n, queries, q_len, q_stride, (int64_t)m, rc, oc, stride)
                      : affine ? drm_sw_align_affine(rt, &affine->scoring, affine->flank, w.data(), q.data(), (int64_t)n,
                                                     queries, q_len, q_stride, (int64_t)m, rc, oc, stride)
                             : drm_sw_align(rt, w.data(), q.data(), (int64_t)n, queries, q_len, q_stride, (int64_t)m, rc,
                                            oc, stride));
            },
            [&](size_t p, const drm_sw_alignment &r, const uint32_t *o) {
                rec[(size_t)row[p]] = r;
                off[(size_t)row[p]] = (int64_t)ops.size();
                ops.insert(ops.end(), o, o + r.n_ops);
            });
        if (affine) {
            for (size_t p = 0; p < np; ++p) {
                int32_t rev = 0;
                check(drm_sw_align_region(rt, wid[p], affine->flank, &region_start[(size_t)row[p]],
                                          &region_len[(size_t)row[p]], &rev));
            }
        }
        if (!want_md)
            return;
        // DRM_SAM_MD: the MD words of the rows just aligned, over the pass's own flank
        std::vector<drm_sw_alignment> r;
        std::vector<int64_t> o;
        two_pass<drm_sw_md>(
            np, 2 * (ref_len + 2 * flank) + 1,
            [&](const size_t *sub, size_t n, int32_t stride, drm_sw_md *h, uint32_t *words) {
                gather(sub, n);
                r.resize(n);
                o.resize(n);
                for (size_t x = 0; x < n; ++x) {
                    r[x] = rec[(size_t)row[sub[x]]];
                    o[x] = off[(size_t)row[sub[x]]];
                }
                check(drm_sw_align_md(rt, flank, w.data(), q.data(), (int64_t)n, queries, q_len, q_stride, (int64_t)m,
                                      r.data(), ops.data(), o.data(), h, words, stride));
            },
            [&](size_t p, const drm_sw_md &h, const uint32_t *words) {
                // an aligner's own record and words always describe a walk; anything else is a fault of this program
                if (h.status != 0 && h.status != 1)
                    throw drm::Error(DRM_ERR_ARG, "drm_sw_align_md: status " + std::to_string(h.status) + " on a row the "
                                                  "aligner produced");
                md[(size_t)row[p]] = h;
                md_off[(size_t)row[p]] = (int64_t)md_words.size();
                md_words.insert(md_words.end(), words, words + h.n_words);
            });
    }
};

// ------------------------------------------------------------------------------------------------ options
// Every numeric DRM_* option is parsed strictly: a non-negative decimal of at most nine digits ...
static bool parse_int(const std::string &t, long &v)
{
    if (t.empty() || t.size() > 9 || t.find_first_not_of("0123456789") != std::string::npos)
        return false;
    v = std::stol(t);
    return true;
}

// ... or a comma list of them: the first n fields into v; returns the number of fields, -1 when one is no such integer
static long parse_int_list(const std::string &s, size_t n, long *v)
{
    size_t count = 0;
    for (size_t p = 0; p <= s.size(); ++count) {
        const size_t q = std::min(s.find(',', p), s.size());
        long x = 0;
        if (!parse_int(s.substr(p, q - p), x))
            return -1;
        if (count < n)
            v[count] = x;
        p = q + 1;
    }
    return (long)count;
}

static std::string quoted(const std::string &s) { return "\"" + s + "\""; }

static bool env_flag(const char *name) { return std::getenv(name) && std::atoi(std::getenv(name)) != 0; }

// `name`, when set, into v: an integer in [lo, 2^20]
static void env_int(const char *name, long lo, int32_t &v)
{
    const char *e = std::getenv(name);
    if (!e)
        return;
    long x = 0;
    if (!parse_int(e, x) || x < lo || x > (1L << 20))
        throw drm::Error(DRM_ERR_ARG, std::string(name) + " must be an integer in [" + std::to_string(lo) +
                                          ", 2^20]: " + quoted(e));
    v = (int32_t)x;
}

// DRM_SAM_SCORING=match,mismatch,open,extend and DRM_SAM_FLANK=n (with DRM_SAM_CIGAR=1 only): strictly parsed, and
// checked against drm_sw_align_affine's ranges (drm::check_scoring) before any work. A flank alone means the scoring
// 1,1,0,1. DRM_SAM_CLIP=L, as strictly: 0..63, drm_sw_clip's range; a penalty above 0 turns the mode on as a flank does,
// and 0 is the unset variable.
static bool affine_mode_from_env(size_t ref_len, AffineMode &mode)
{
    const char *sc = std::getenv("DRM_SAM_SCORING"), *fl = std::getenv("DRM_SAM_FLANK");
    const char *cl = std::getenv("DRM_SAM_CLIP");
    long clip = 0;
    if (cl && (!parse_int(cl, clip) || clip > 63))
        throw drm::Error(DRM_ERR_ARG, "DRM_SAM_CLIP must be an integer in [0, 63]: " + quoted(cl));
    if (!sc && !fl && clip == 0)
        return false;
    mode = AffineMode{{1, 1, 0, 1}, 0, (int32_t)clip};
    if (sc) {
        long v[4] = {};
        const long n = parse_int_list(sc, 4, v);
        if (n < 0)
            throw drm::Error(DRM_ERR_ARG, "DRM_SAM_SCORING must be match,mismatch,open,extend (four non-negative "
                                          "integers): " + quoted(sc));
        mode.scoring = drm_sw_scoring{(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3]};
        bool in_range = n == 4;
        try {
            drm::check_scoring(&mode.scoring); // the ranges are the library's, the text names the variable
        } catch (const drm::Error &) {
            in_range = false;
        }
        if (!in_range)
            throw drm::Error(DRM_ERR_ARG, "DRM_SAM_SCORING must be match,mismatch,open,extend with match 1..31, "
                                          "mismatch 1..63, open 0..63, extend 1..63: " + quoted(sc));
    }
    if (fl) {
        long x = 0;
        if (!parse_int(fl, x))
            throw drm::Error(DRM_ERR_ARG, "DRM_SAM_FLANK must be a non-negative integer: " + quoted(fl));
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
// DRM_PAIR_TLEN=auto instead of min,max: the window is estimated from the first DRM_PAIR_TLEN_SAMPLE=n pairs (default
// 65,536, 1 to 2^24) before the block loop, from the pairs whose mates both reach MAPQ DRM_PAIR_TLEN_MAPQ=n (default
// 20, 0 to 60) on their own (Pipeline::estimate_tlen); both variables are read only then, as strictly. The rescue's cap
// is then checked on the estimated window.
constexpr int32_t kRescueMinDefault = 49; // the largest chance score measured, 39, plus 10
constexpr int32_t kRescueMaxRows = 2048;  // drm_mate_rescue's cap on dhi - dlo + ref_len
constexpr int32_t kTlenMinSamples = 10;   // bwa-mem's
struct PairMode {
    std::string mates;
    drm_pair_params prm;
    bool rescue = false;
    int32_t rescue_min = kRescueMinDefault;
    bool tlen_auto = false;
    size_t tlen_sample = (size_t)1 << 16;
    int32_t tlen_mapq = 20;
};

// `name`, when set, into v: an integer in [lo, hi]
static void env_range(const char *name, long lo, long hi, long &v)
{
    const char *e = std::getenv(name);
    if (!e)
        return;
    long x = 0;
    if (!parse_int(e, x) || x < lo || x > hi)
        throw drm::Error(DRM_ERR_ARG, std::string(name) + " must be an integer in [" + std::to_string(lo) + ", " +
                                          std::to_string(hi) + "]: " + quoted(e));
    v = x;
}

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
    const char *tl = std::getenv("DRM_PAIR_TLEN");
    if (tl && std::string(tl) == "auto") {
        long n = (long)mode.tlen_sample, q = mode.tlen_mapq;
        env_range("DRM_PAIR_TLEN_SAMPLE", 1, 1L << 24, n);
        env_range("DRM_PAIR_TLEN_MAPQ", 0, 60, q);
        mode.tlen_auto = true;
        mode.tlen_sample = (size_t)n;
        mode.tlen_mapq = (int32_t)q;
    } else if (tl) {
        long v[2] = {};
        if (parse_int_list(tl, 2, v) != 2)
            throw drm::Error(DRM_ERR_ARG, "DRM_PAIR_TLEN must be min,max (two non-negative integers): " + quoted(tl));
        if (v[0] > v[1] || v[1] > (1L << 30))
            throw drm::Error(DRM_ERR_ARG, "DRM_PAIR_TLEN must be min,max with 0 <= min <= max <= 2^30: " + quoted(tl));
        mode.prm.min_tlen = (int32_t)v[0];
        mode.prm.max_tlen = (int32_t)v[1];
    }
    env_int("DRM_PAIR_PENALTY", 0, mode.prm.unpaired_penalty);
    mode.rescue = env_flag("DRM_PAIR_RESCUE");
    if (mode.rescue) {
        env_int("DRM_PAIR_RESCUE_MIN", 0, mode.rescue_min);
        int64_t dlo = 0, dhi = 0;
        if (!mode.tlen_auto)
            drm::check_rescue_params(&mode.prm, dlo, dhi); // DRM_PAIR_TLEN wider than the rescue's 2,048 rows
    }
    return true;
}

// DRM_SAM_MAPQ=1 (with use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1 only): the MAPQ column comes from the locus scan of
// each read's rerank rows (drm_hit_mapq, drm_pair_mapq) instead of the constant 60. DRM_MAPQ_MIN=n (default 39, the
// largest chance score DESIGN.md sec. 4.11 recorded for 150-base reads) and DRM_MAPQ_SPAN=n (default ref_len) are read
// only then, as strictly as DRM_SAM_SCORING; sub_band is 2, one substitution under the rerank's scoring {1, 1, 0, 1}.
// DRM_PAIR_TLEN=auto scans with the same parameters, whether or not DRM_SAM_MAPQ is on.
constexpr int32_t kMapqMinDefault = 39;
static drm_mapq_params mapq_params_from_env(size_t ref_len)
{
    drm_mapq_params prm{(int32_t)ref_len, (int32_t)ref_len, kMapqMinDefault, 2};
    env_int("DRM_MAPQ_MIN", 0, prm.min_score);
    env_int("DRM_MAPQ_SPAN", 1, prm.locus_span);
    return prm;
}

static bool mapq_mode_from_env(size_t ref_len, bool l2_rows, drm_mapq_params &prm)
{
    if (!env_flag("DRM_SAM_MAPQ"))
        return false;
    if (ref_len < 1 || ref_len > ((size_t)1 << 20))
        throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_SAM_MAPQ: ref_len " + std::to_string(ref_len) + " outside [1, 2^20]");
    prm = mapq_params_from_env(ref_len);
    if (l2_rows)
        throw drm::Error(DRM_ERR_ARG, "DRM_SAM_MAPQ does not go with DRM_SAM_L2_ROWS=1: those rows carry distances, "
                                      "not scores");
    return true;
}

// DRM_SAM_LOCI=n (1..64, with DRM_SAM_MAPQ=1 and everything that needs): one SAM line per distinct locus of a read
// instead of one per rerank row, from drm_hit_loci with max_loci = n. DRM_LOCI_DROP=pct (default 80, bwa-mem's XA drop
// ratio: a default, not a measurement) is read only then. DRM_SAM_XA=1 beside it folds the alternative loci into an
// XA:Z tag on the primary line; pairs always take that form. All three are parsed as strictly as DRM_SAM_SCORING.
constexpr int32_t kLociDropDefault = 80;
static bool loci_mode_from_env(bool mapq, drm_loci_params &prm, bool &xa)
{
    const char *e = std::getenv("DRM_SAM_LOCI"), *x = std::getenv("DRM_SAM_XA");
    long n = 0, drop = kLociDropDefault, flag = 0;
    env_range("DRM_SAM_XA", 0, 1, flag);
    xa = flag != 0;
    if (!e) {
        if (xa)
            throw drm::Error(DRM_ERR_ARG, "DRM_SAM_XA needs DRM_SAM_LOCI=n: the tag lists the loci it finds: " + quoted(x));
        return false;
    }
    env_range("DRM_SAM_LOCI", 1, 64, n);
    env_range("DRM_LOCI_DROP", 0, 100, drop);
    if (!mapq)
        throw drm::Error(DRM_ERR_ARG, "DRM_SAM_LOCI needs DRM_SAM_MAPQ=1 (with use_dynamic=1 use_streaming=1 "
                                      "DRM_SAM_CIGAR=1 and sequence queries): the loci come from the MAPQ's scan");
    prm = drm_loci_params{(int32_t)n, (int32_t)drop};
    return true;
}

// What one run does, from argv and every DRM_* variable this file reads; nothing after read_options calls getenv.
struct Options {
    std::string query_file, ref_file, out_dir, sam_file;
    std::string model; // the GRU model of a sequence input (drm::encoder_model_path), empty = the 3-mer stand-in
    size_t ref_len = 0, stride = 0;
    int ef = 128, k = 128, k_clusters = 5;
    bool use_streaming = false, is_npy = false;
    bool dyn = false; // windows cut from the genome string on the device
    bool has_affine = false, paired = false, mapq = false;
    bool contigs = false; // DRM_CONTIGS: the reference's contigs are told apart (Pipeline::contig_stage)
    AffineMode affine_mode{};
    PairMode pair{};
    drm_mapq_params mapq_prm{};
    bool loci = false, sam_xa = false; // DRM_SAM_LOCI: lines per locus (drm_hit_loci); DRM_SAM_XA: alternates as XA:Z
    drm_loci_params loci_prm{};
    std::vector<int> devices;
    // the output mode: the first that holds of header_only, l2_rows, paired, stream_sam; none = the .npy files
    bool stream_sam = false, header_only = false, l2_rows = false;
    bool sam_from_search = false, sam_cigar = false, l2_rows_from_sw = false;
    bool sam_md = false;   // DRM_SAM_MD: MD:Z behind NM:i on every mapped line of the DRM_SAM_CIGAR modes
    bool sam_qual = false; // DRM_SAM_QUAL: column 11 from the FASTQ's quality lines
    bool sam_stats = false; // DRM_SAM_STATS: one line with the SAM stage's time and the rows it aligned
    bool sam_dup = false;   // DRM_SAM_DUP: flag 1024 on the lines of a template whose 5' ends were seen before
    bool sam_sort = false;  // DRM_SAM_SORT=coordinate: the lines are held back and written in coordinate order
    bool sam_bam = false;   // DRM_SAM_FORMAT=bam: results.bam (BAM records, BGZF from the device) instead of results.sam
    size_t sam_block = 0; // DRM_SAM_BLOCK, 0 = unset

    const AffineMode *affine() const { return has_affine ? &affine_mode : nullptr; }
    // rows of one alignment pass: DRM_SAM_BLOCK when set, else blocks of about 4M rows
    size_t block(size_t rows_per_query) const
    {
        const size_t rows = ((size_t)1 << 22) / std::max<size_t>(rows_per_query, 1);
        return sam_block ? sam_block : sam_cigar ? std::clamp<size_t>(rows, 1, 1u << 20) : 1u << 20;
    }
};

static Options read_options(int argc, char *argv[], size_t ref_len, size_t stride)
{
    Options o;
    o.ref_len = ref_len;
    o.stride = stride;
    o.query_file = argv[2];
    o.ref_file = argv[3];
    auto number = [&](int i, int absent) { return argc > i ? std::stoi(argv[i]) : absent; };
    o.ef = number(4, 128);
    o.k = number(5, 128);
    o.k_clusters = stride == 1 ? o.k : number(6, 5);
    o.out_dir = argc >= 8 ? argv[7] : ".";
    const bool use_dynamic = number(8, 0) != 0;
    o.use_streaming = number(9, 0) != 0;
    o.sam_file = o.out_dir + "/results.sam"; // src/main.cpp:67
    o.is_npy = std::filesystem::path(o.query_file).extension() == ".npy";
    const bool cigar = env_flag("DRM_SAM_CIGAR"), l2_rows = env_flag("DRM_SAM_L2_ROWS");
    o.has_affine = cigar && affine_mode_from_env(ref_len, o.affine_mode);
    o.paired = pair_mode_from_env(ref_len, o.pair);
    o.mapq = use_dynamic && o.use_streaming && cigar && !o.is_npy && mapq_mode_from_env(ref_len, l2_rows, o.mapq_prm);
    if (!o.paired && std::getenv("DRM_PAIR_TLEN") && std::string(std::getenv("DRM_PAIR_TLEN")) == "auto")
        throw drm::Error(DRM_ERR_ARG, "DRM_PAIR_TLEN=auto needs DRM_MATES: the window is estimated from read pairs");
    if (o.paired && o.pair.tlen_auto && !o.mapq)
        o.mapq_prm = mapq_params_from_env(ref_len);
    if (o.paired) {
        if (!use_dynamic || !o.use_streaming)
            throw drm::Error(DRM_ERR_ARG, "DRM_MATES needs use_dynamic=1 and use_streaming=1: pairs are written to the "
                                          "streamed SAM");
        if (!cigar)
            throw drm::Error(DRM_ERR_ARG, "DRM_MATES needs DRM_SAM_CIGAR=1: the pair fields come from real alignments");
        if (o.is_npy || std::filesystem::path(o.pair.mates).extension() == ".npy")
            throw drm::Error(DRM_ERR_ARG, "DRM_MATES needs sequence files for both mates, not .npy embeddings");
    }
    // devices: DRM_DEVICES=0,1,... fans the batch out over several GPUs (contiguous query shards,
    // replicated index); DRM_DEVICE=i picks one (default 0)
    if (const char *dl = std::getenv("DRM_DEVICES")) {
        std::istringstream fields(dl);
        for (std::string t; std::getline(fields, t, ',');)
            if (!t.empty())
                o.devices.push_back(std::stoi(t));
    }
    if (o.devices.empty())
        o.devices.push_back(std::getenv("DRM_DEVICE") ? std::atoi(std::getenv("DRM_DEVICE")) : 0);
    if (o.paired && o.devices.size() != 1)
        throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_MATES runs on one device (DRM_DEVICE), not on DRM_DEVICES");
    if (o.mapq && o.devices.size() != 1)
        throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_SAM_MAPQ runs on one device (DRM_DEVICE), not on DRM_DEVICES");
    o.loci = loci_mode_from_env(o.mapq, o.loci_prm, o.sam_xa);
    // DRM_CONTIGS=1: everything it needs is checked here, before the index is loaded
    o.contigs = env_flag("DRM_CONTIGS");
    if (o.contigs) {
        if (!use_dynamic || !o.use_streaming)
            throw drm::Error(DRM_ERR_ARG, "DRM_CONTIGS needs use_dynamic=1 and use_streaming=1: contigs are told apart "
                                          "in the streamed SAM");
        if (!cigar)
            throw drm::Error(DRM_ERR_ARG, "DRM_CONTIGS needs DRM_SAM_CIGAR=1: RNAME and POS come from real alignments");
        if (o.is_npy)
            throw drm::Error(DRM_ERR_ARG, "DRM_CONTIGS needs sequence queries, not .npy embeddings");
        if (o.devices.size() != 1)
            throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_CONTIGS runs on one device (DRM_DEVICE), not on DRM_DEVICES");
        if (stride != 1)
            throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_CONTIGS needs an index of stride 1, not " +
                                                      std::to_string(stride));
        if (l2_rows)
            throw drm::Error(DRM_ERR_ARG, "DRM_CONTIGS does not go with DRM_SAM_L2_ROWS=1");
        if (ref_len < 1 || ref_len > ((size_t)1 << 20))
            throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_CONTIGS: ref_len " + std::to_string(ref_len) +
                                                      " outside [1, 2^20]");
    }
    o.sam_md = env_flag("DRM_SAM_MD");
    if (o.sam_md && !cigar)
        throw drm::Error(DRM_ERR_ARG, "DRM_SAM_MD needs DRM_SAM_CIGAR=1: MD describes a real alignment");
    o.sam_qual = env_flag("DRM_SAM_QUAL");
    o.sam_stats = env_flag("DRM_SAM_STATS");
    // DRM_SAM_DUP=0|1, parsed as strictly as DRM_SAM_XA; everything it needs is checked here, before the index is loaded
    long dup_flag = 0;
    env_range("DRM_SAM_DUP", 0, 1, dup_flag);
    o.sam_dup = dup_flag != 0;
    if (o.sam_dup && !(cigar && (o.paired || o.loci)))
        throw drm::Error(DRM_ERR_ARG, "DRM_SAM_DUP needs DRM_SAM_CIGAR=1 with DRM_MATES or DRM_SAM_LOCI (and all they "
                                      "need): a template is keyed by the one primary placement of each of its reads");
    if (const char *e = std::getenv("DRM_SAM_BLOCK"))
        o.sam_block = std::max<size_t>(1, std::strtoull(e, nullptr, 10));
    // DRM_SAM_SORT=unsorted|coordinate, nothing else; everything it needs is checked here, before the index is loaded
    if (const char *e = std::getenv("DRM_SAM_SORT")) {
        const std::string v = e;
        if (v != "unsorted" && v != "coordinate")
            throw drm::Error(DRM_ERR_ARG, "DRM_SAM_SORT must be unsorted or coordinate: " + quoted(v));
        o.sam_sort = v == "coordinate";
        if (o.sam_sort && !(use_dynamic && o.use_streaming && cigar && !o.is_npy))
            throw drm::Error(DRM_ERR_ARG, "DRM_SAM_SORT=coordinate needs use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1 "
                                          "and sequence queries: the keys are the lines' real RNAME and POS");
    }
    // DRM_SAM_FORMAT=sam|bam, nothing else; checked like DRM_SAM_SORT, before the index is loaded
    if (const char *e = std::getenv("DRM_SAM_FORMAT")) {
        const std::string v = e;
        if (v != "sam" && v != "bam")
            throw drm::Error(DRM_ERR_ARG, "DRM_SAM_FORMAT must be sam or bam: " + quoted(v));
        o.sam_bam = v == "bam";
        if (o.sam_bam && !(use_dynamic && o.use_streaming && cigar && !o.is_npy))
            throw drm::Error(DRM_ERR_ARG, "DRM_SAM_FORMAT=bam needs use_dynamic=1 use_streaming=1 DRM_SAM_CIGAR=1 and "
                                          "sequence queries: the records hold the lines' real RNAME, POS and CIGAR");
        if (o.sam_bam && o.devices.size() != 1)
            throw drm::Error(DRM_ERR_UNSUPPORTED, "DRM_SAM_FORMAT=bam runs on one device (DRM_DEVICE), not on "
                                                  "DRM_DEVICES");
        if (o.sam_bam)
            o.sam_file = o.out_dir + "/results.bam";
    }
    if (!o.is_npy)
        o.model = drm::encoder_model_path();

    // The reference streams its SAM from post_process_l2_dynamic_streaming (src/main.cpp:316-319). With a
    // dense index (stride 1) that function skips every reranker and writes the first min(k, k_clusters)
    // search neighbours of each query in search order (src/utils/post_processor.cpp:833-878), so the SAM
    // here comes straight from the search and no rerank runs. A sparse index reranks the expanded windows of
    // the whole run by L2 (:884-1010): drm_post_process_l2_dynamic over every query after the search, on a
    // window-embedding table of the genome built by the GRU model. Without the model (3-mer stand-in) or
    // across several devices, those SAM rows come from the SW rerank instead. (What the sparse branch really
    // writes: Pipeline::write_sparse_sam.)
    o.dyn = use_dynamic && !o.is_npy;
    o.stream_sam = o.use_streaming && o.dyn;
    // DRM_MATES, DRM_SAM_MAPQ: pairing and MAPQ need scores, so the SW rerank runs whatever the stride
    // DRM_CONTIGS: the contig stage works on the rerank's rows, so the rerank runs as well
    o.sam_from_search = o.stream_sam && stride == 1 && !o.paired && !o.mapq && !o.contigs;
    const bool sparse_rows = o.stream_sam && stride > 1 && l2_rows && !o.paired;
    o.header_only = o.stream_sam && stride > 1 && !l2_rows && !o.paired && !o.mapq;
    o.l2_rows = sparse_rows && o.devices.size() == 1 && !o.model.empty();
    o.l2_rows_from_sw = sparse_rows && !o.l2_rows;
    // DRM_SAM_CIGAR=1: every SAM row gets its real POS / CIGAR / AS / NM from a GPU
    // alignment of the block's rows (drm_sw_align) before the host thread formats the block. Unset: no
    // alignment is launched and the file is the reference's.
    o.sam_cigar = o.stream_sam && !o.header_only && cigar;
    if (o.sam_sort && (o.header_only || l2_rows))
        throw drm::Error(DRM_ERR_ARG, "DRM_SAM_SORT=coordinate does not go with a sparse index's header-only SAM or "
                                      "DRM_SAM_L2_ROWS=1: those files are not written by the block loop");
    if (o.sam_bam && (o.header_only || l2_rows))
        throw drm::Error(DRM_ERR_ARG, "DRM_SAM_FORMAT=bam does not go with a sparse index's header-only SAM or "
                                      "DRM_SAM_L2_ROWS=1: those files are not written by the block loop");
    return o;
}

// a read's self score under the rerank's scoring: its length without format_fastq's tags
static int32_t untagged_length(const std::string &tagged)
{
    const int pre = !tagged.empty() && tagged.front() == '<', post = tagged.size() > 1 && tagged.back() == '>';
    return (int32_t)tagged.size() - pre - post;
}

// DRM_MATES: mate 1 of pair i becomes query 2i, mate 2 query 2i + 1, both under mate 1's name
// (DRM_SAM_QUAL, quals non-null: the quality lines travel with their reads)
static void interleave_mates(const std::string &query_file, const std::string &mates, std::vector<std::string> &qseqs,
                             std::vector<std::string> &qids, std::vector<std::string> *quals)
{
    std::vector<std::string> seqs2, ids2, quals2;
    if (quals)
        drm::read_file_qual(mates, seqs2, ids2, quals2);
    else
        drm::read_file(mates, seqs2, ids2);
    const size_t n1 = qseqs.size(), n2 = seqs2.size();
    auto name = [](const std::vector<std::string> &ids, size_t i) { return i < ids.size() ? ids[i] : std::string(); };
    for (size_t i = 0; i < std::min(n1, n2); ++i)
        if (name(qids, i) != name(ids2, i))
            throw drm::Error(DRM_ERR_FORMAT, "DRM_MATES: record " + std::to_string(i) + " is named \"" + name(qids, i) +
                                                 "\" in " + query_file + " and \"" + name(ids2, i) + "\" in " + mates);
    if (n1 != n2)
        throw drm::Error(DRM_ERR_FORMAT, "DRM_MATES: " + query_file + " has " + std::to_string(n1) + " records and " +
                                             mates + " has " + std::to_string(n2) + ": record " +
                                             std::to_string(std::min(n1, n2)) + " has no mate");
    std::vector<std::string> seqs(2 * n1), ids(2 * n1);
    for (size_t i = 0; i < n1; ++i) {
        seqs[2 * i] = std::move(qseqs[i]);
        seqs[2 * i + 1] = std::move(seqs2[i]);
        ids[2 * i] = ids[2 * i + 1] = name(qids, i);
    }
    qseqs.swap(seqs);
    qids.swap(ids);
    if (quals && (!quals->empty() || !quals2.empty())) { // a mate file without quality lines (.txt) keeps "*"
        std::vector<std::string> both(2 * n1);
        for (size_t i = 0; i < n1; ++i) {
            if (i < quals->size())
                both[2 * i] = std::move((*quals)[i]);
            if (i < quals2.size())
                both[2 * i + 1] = std::move(quals2[i]);
        }
        quals->swap(both);
    }
    std::cout << "[MAIN] Paired mode: " << n1 << " pairs, mates from " << mates << std::endl;
}

// ------------------------------------------------------------------------------------------------ the run
// One run's state; main calls the stages in order.
struct Pipeline {
    const Options &o;
    const size_t k, kc; // o.k, o.k_clusters as row widths
    // queries: embeddings (.npy input) or sequences, qs = the longest sequence
    drm::NpyArray emb;
    size_t nq = 0, dim = 0, qs = 0;
    std::vector<std::string> qseqs, qids;
    std::vector<std::string> quals; // DRM_SAM_QUAL: the reads' quality lines, empty = "*" on every line
    // reference: the static window table as one fixed-width block, or the genome string
    size_t n_ref = 0;
    std::string table, genome;
    // one index replica per device; art is the handle the alignments run on (several devices: one more genome
    // handle on the first)
    drm_index *index = nullptr;
    drm_refs *rt = nullptr, *art = nullptr;
    drm_multi *multi = nullptr;
    drm_index_info info{};
    int device = 0;
    // pinned inputs and outputs of the search + rerank
    Pinned<float> x, D;
    Pinned<uint8_t> qbuf;
    Pinned<int32_t> ql, status, sw_scores;
    Pinned<int64_t> I;
    Pinned<uint64_t> sw_ids;
    drm_search_stats st{};
    // DRM_CONTIGS: the reference's contig table, its handle, and per rerank row [nq x k] the spread id and the contig that
    // contig_stage leaves beside the filtered sw_ids / sw_scores / status
    std::vector<drm::FastaContig> ctable;
    drm_contigs *ctg = nullptr;
    std::vector<uint64_t> spread;
    std::vector<int32_t> row_contig;
    drm_pair_params pair_prm; // o.pair.prm, with DRM_PAIR_TLEN=auto the estimated window from estimate_tlen on
    drm_dupset *dups = nullptr; // DRM_SAM_DUP: the run's first-seen set, one item per pair or read (run)
    // DRM_SAM_SORT=coordinate: every line of the run with its key, filled by the writer thread block after block
    mutable drm::SamSpool spool;
    // DRM_SAM_FORMAT=bam: the run's BAM file, fed by the writer thread block after block and closed by run()
    mutable drm::BamFile bam;
    // DRM_SAM_STATS: the rows handed to the aligner and the time of the blocks' produce steps (everything between the
    // rerank and the writer thread: the locus scans, the alignments, the MD pass)
    size_t aligned_rows = 0;
    double produce_ms = 0;

    explicit Pipeline(const Options &opt)
        : o(opt), k((size_t)opt.k), kc((size_t)opt.k_clusters), device(opt.devices[0]), pair_prm(opt.pair.prm)
    {
        bam.device = device;
    }

    // false: a sequence file without a record
    bool load_queries()
    {
        if (o.is_npy) {
            emb = drm::npy_load(o.query_file);
            if (emb.shape.size() != 2)
                throw drm::Error(DRM_ERR_FORMAT, "Error: Expected 2D array in .npy file");
            if (emb.kind != 'f' || emb.itemsize != 4)
                throw drm::Error(DRM_ERR_FORMAT, "embeddings .npy must be float32 ('<f4')");
            nq = emb.shape[0];
            dim = emb.shape[1];
            std::cout << "[MAIN] Loaded " << nq << " embeddings of dimension " << dim << std::endl;
            return true;
        }
        if (o.sam_qual)
            drm::read_file_qual(o.query_file, qseqs, qids, quals);
        else
            drm::read_file(o.query_file, qseqs, qids);
        if (qseqs.empty()) {
            std::cerr << "No query_sequences found in input file!" << std::endl;
            return false;
        }
        if (o.paired)
            interleave_mates(o.query_file, o.pair.mates, qseqs, qids, o.sam_qual ? &quals : nullptr);
        nq = qseqs.size();
        for (auto &q : qseqs)
            qs = std::max(qs, q.size());
        return true;
    }

    // the static window table (read_file(ref, ref_len, 1, lookup)), or with use_dynamic the genome string
    // (extract_FASTA_sequence), windows cut on the device (src/main.cpp:182-192)
    void load_reference()
    {
        if (o.dyn) {
            std::cout << "[MAIN] Using DYNAMIC fetching for reference sequences" << std::endl;
            genome = drm::extract_fasta_sequence(o.ref_file);
            std::cout << "[MAIN] Loaded a " << genome.size() << " bp genome from " << o.ref_file << std::endl;
            if (o.contigs) {
                ctable = drm::fasta_contigs(o.ref_file);
                std::cout << "[MAIN] DRM_CONTIGS: " << ctable.size() << " contigs" << std::endl;
            }
        } else if (!o.is_npy) {
            std::cout << "[MAIN] Using STATIC fetching for reference sequences" << std::endl;
            std::vector<std::string> refs, dummy;
            drm::read_file(o.ref_file, refs, dummy, o.ref_len, 1, true);
            std::cout << "[MAIN] Loaded " << refs.size() << " reference sequences from " << o.ref_file << std::endl;
            // the device window table is fixed-width: a .txt / .fastq reference whose lines are not
            // all ref_len bytes would be over-read or silently truncated (the reference scores the
            // whole string), so it is refused before anything touches the GPU
            for (size_t r = 0; r < refs.size(); ++r)
                if (refs[r].size() != o.ref_len)
                    throw drm::Error(DRM_ERR_FORMAT, "reference sequence " + std::to_string(r) + " has " +
                                                         std::to_string(refs[r].size()) +
                                                         " bytes; the window table needs ref_len = " +
                                                         std::to_string(o.ref_len) + " for every window");
            n_ref = refs.size();
            table.assign(n_ref * o.ref_len, '\0');
            for (size_t r = 0; r < n_ref; ++r)
                std::memcpy(&table[r * o.ref_len], refs[r].data(), o.ref_len);
        }
    }

    drm_refs *genome_handle()
    {
        drm_refs *h = nullptr;
        check(drm_refs_create_genome((const uint8_t *)genome.data(), (int64_t)genome.size(), (int32_t)o.ref_len, device,
                                     &h));
        return h;
    }

    // the index (one replica per device), the reference handle and the executor's buffers
    void open(const std::string &index_file)
    {
        const auto t0 = clk::now();
        if (!std::filesystem::exists(index_file))
            throw drm::Error(DRM_ERR_IO, "Index file does not exist: " + index_file);
        const uint8_t *tbl = o.is_npy ? nullptr : (const uint8_t *)table.data();
        const std::vector<int> &devices = o.devices;
        if (devices.size() == 1) {
            check(drm_index_load(index_file.c_str(), device, &index));
            check(drm_index_get_info(index, &info));
            if (o.dyn)
                rt = genome_handle();
            else if (!o.is_npy)
                check(drm_refs_create(tbl, (int64_t)n_ref, (int32_t)o.ref_len, (int64_t)o.ref_len, device, &rt));
        } else {
            if (o.dyn)
                check(drm_multi_create_genome(index_file.c_str(), devices.data(), (int)devices.size(),
                                              (const uint8_t *)genome.data(), (int64_t)genome.size(),
                                              (int32_t)o.ref_len, &multi));
            else
                check(drm_multi_create(index_file.c_str(), devices.data(), (int)devices.size(), tbl, (int64_t)n_ref,
                                       (int32_t)o.ref_len, (int64_t)o.ref_len, &multi));
            check(drm_multi_get_index_info(multi, &info));
        }
        if (o.contigs) {
            const int64_t want = genome.size() >= o.ref_len ? 2 * (int64_t)(genome.size() - o.ref_len + 1) : 0;
            if (info.ntotal != want)
                throw drm::Error(DRM_ERR_ARG, "DRM_CONTIGS: the index holds " + std::to_string(info.ntotal) +
                                                  " vectors, the genome string of " + o.ref_file + " has " +
                                                  std::to_string(want) + " windows: rebuild the index with DRM_CONTIGS=1");
            std::vector<int64_t> starts, lens;
            for (const drm::FastaContig &c : ctable) {
                starts.push_back(c.start);
                lens.push_back(c.len);
            }
            check(drm_contigs_create(starts.data(), lens.data(), (int64_t)starts.size(), device, &ctg));
        }
        if (index) // the executor's streams and buffers for this batch, outside the search timing
            check(drm_search_rerank_prepare(index, (int64_t)nq, (int32_t)(o.is_npy ? dim : info.d), o.k_clusters, o.k,
                                            o.is_npy ? 0 : (int32_t)qs));
        std::cout << "[MAIN] Index loaded time: " << ms_since(t0) << " ms (" << info.ntotal << " vectors, "
                  << info.device_bytes / (1 << 20) << " MiB on each of " << devices.size() << " device(s))"
                  << std::endl;
    }

    // Vectorizer::vectorize (src/main.cpp:249-268), into pinned host memory: the GRU model on the GPU (DRM_ENCODER
    // or the reference's models/ path), else the deterministic 3-mer stand-in
    void embed()
    {
        if (!o.is_npy)
            dim = (size_t)info.d;
        x.alloc(nq * dim);
        if (o.is_npy) {
            std::memcpy(x.p, emb.bytes.data(), sizeof(float) * nq * dim);
            return;
        }
        const auto t0 = clk::now();
        if (!o.model.empty()) {
            if (dim != 128)
                throw drm::Error(DRM_ERR_ARG,
                                 "the GRU model emits 128-d embeddings; the index has d = " + std::to_string(dim));
            drm::vectorize_host(o.model, device, qseqs, x.p);
            std::cout << "[MAIN] Inference (GRU model " << o.model << ", GPU) time: " << ms_since(t0) << " ms"
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
    }

    // the pinned query bytes and result arrays of the search + rerank
    void alloc_buffers()
    {
        qbuf.alloc(nq * std::max<size_t>(qs, 1));
        ql.alloc(nq);
        status.alloc(nq);
        for (size_t i = 0; i < nq && !o.is_npy; ++i) {
            std::memset(qbuf.p + i * qs, 0, qs);
            std::memcpy(qbuf.p + i * qs, qseqs[i].data(), qseqs[i].size());
            ql.p[i] = (int32_t)qseqs[i].size();
        }
        D.alloc(nq * kc);
        I.alloc(nq * kc);
        sw_scores.alloc(o.is_npy ? 0 : nq * k);
        sw_ids.alloc(o.is_npy ? 0 : nq * k);
        if (o.contigs) {
            spread.assign(nq * k, ~0ull);
            row_contig.assign(nq * k, -1);
        }
    }

    // DRM_CONTIGS, after the search + rerank of reads [lo, lo + m): drm_contig_hits over their rows. The stage's lists and
    // counts replace the rerank's in sw_ids / sw_scores / status, so that everything downstream reads real ids of rows
    // inside one contig; the spread ids and the contigs go beside them.
    void contig_stage(size_t lo, size_t m)
    {
        std::vector<uint64_t> ids(m * k);
        std::vector<int32_t> sc(m * k), cnt(m);
        check(drm_contig_hits(ctg, (int32_t)o.ref_len, sw_ids.p + lo * k, sw_scores.p + lo * k, status.p + lo, (int64_t)m,
                              o.k, ids.data(), spread.data() + lo * k, sc.data(), row_contig.data() + lo * k, cnt.data()));
        std::memcpy(sw_ids.p + lo * k, ids.data(), sizeof(uint64_t) * m * k);
        std::memcpy(sw_scores.p + lo * k, sc.data(), sizeof(int32_t) * m * k);
        std::memcpy(status.p + lo, cnt.data(), sizeof(int32_t) * m);
    }
    // the ids the pair-level kernels get: the spread ids under DRM_CONTIGS
    const uint64_t *level_ids() const { return o.contigs ? spread.data() : sw_ids.p; }

    // HNSW search (faiss_search(alg_hnsw, embeddings, k_clusters, ef), src/main.cpp:278) streamed into the SW rerank
    // (post_process_sw_static, :333-341) batch by batch: one pass over queries [lo, lo + m) into the output arrays at
    // row lo
    int search(size_t lo, size_t m, drm_search_stats *sp)
    {
        const bool search_only = o.sam_from_search || o.l2_rows || o.header_only;
        const uint8_t *qb = (o.is_npy || search_only) ? nullptr : qbuf.p + lo * qs;
        if (multi)
            return drm_multi_search_rerank(multi, x.p + lo * dim, (int64_t)m, (int32_t)dim, o.k_clusters, o.ef, qb,
                                           ql.p + lo, (int32_t)qs, (int64_t)o.stride, o.k, D.p + lo * kc, I.p + lo * kc,
                                           sw_scores.p + lo * k, sw_ids.p + lo * k, status.p + lo, sp);
        return drm_search_rerank(index, search_only ? nullptr : rt, x.p + lo * dim, (int64_t)m, (int32_t)dim,
                                 o.k_clusters, o.ef, qb, ql.p + lo, (int32_t)qs, (int64_t)o.stride, o.k, D.p + lo * kc,
                                 I.p + lo * kc, sw_scores.p + lo * k, sw_ids.p + lo * k, status.p + lo, sp);
    }

    void open_sam(const char *note = "")
    {
        std::cout << "[MAIN] Using STREAMING output to SAM file: " << o.sam_file << note << std::endl;
        std::filesystem::create_directories(o.out_dir);
    }

    // What every block of the run's SAM file shares, for the block that starts at query q0 (the first one writes the
    // header); the caller adds the block's rows.
    drm::SamBlock sam_block(size_t q0) const
    {
        drm::SamBlock b;
        b.path = o.sam_file;
        b.header = q0 == 0;
        b.ref_len = o.ref_len;
        b.queries = &qseqs;
        b.query_ids = &qids;
        b.quals = &quals;
        b.q0 = q0;
        b.spool = o.sam_sort ? &spool : nullptr;
        b.bam = o.sam_bam ? &bam : nullptr;
        return b;
    }

    // contig: with DRM_CONTIGS the contig of every row, indexed like ids (the flank guard)
    void align_block(BlockAlignments &ba, const uint64_t *ids, const int32_t *cnt, size_t lo, size_t m, size_t width,
                     const int32_t *contig = nullptr, bool md = true)
    {
        ba.want_md = o.sam_md && md;
        for (size_t i = 0; i < m; ++i)
            aligned_rows += (size_t)std::clamp<int64_t>(cnt[i], 0, (int64_t)width);
        ba.align(art, ids, cnt, m, width, qbuf.p + lo * qs, ql.p + lo, (int32_t)qs, (int32_t)o.ref_len, o.affine(),
                 contig ? ctg : nullptr, contig);
    }

    // DRM_SAM_DUP, after the alignment of a block: items [item0, item0 + n) of `per` reads each, block read r having its
    // primary row at r * width of ids / ba and cnt[r] rows. A read whose primary row holds an alignment gives the end
    // word of its unclipped 5' end, over the row's region when the block has regions, else over the window of its id; any
    // other read gives 0. One drm_dupset_mark per block, the blocks being produced in item order; returns per read of the
    // block whether its template is a duplicate.
    std::shared_ptr<std::vector<uint8_t>> mark_duplicates(const BlockAlignments &ba, const uint64_t *ids,
                                                          const int32_t *cnt, size_t lo, size_t item0, size_t n,
                                                          size_t per, size_t width)
    {
        std::vector<uint64_t> ends(2 * n, 0);
        const bool regions = !ba.region_start.empty();
        for (size_t r = 0; r < n * per; ++r) {
            const size_t row = r * width;
            if (cnt[r] < 1 || ba.rec[row].status != 0)
                continue;
            const std::string &tagged = qseqs[lo + r];
            const int32_t rev = (int32_t)(ids[row] & 1u);
            int64_t end5 = 0;
            check(drm_sam_end5(&ba.rec[row], !tagged.empty() && tagged.front() == '<',
                               regions ? ba.region_start[row] : (int64_t)(ids[row] / 2),
                               regions ? ba.region_len[row] : (int32_t)o.ref_len, rev, &end5));
            check(drm_dup_end_word(end5, rev, &ends[2 * (r / per) + (per == 2 ? r % 2 : 0)]));
        }
        std::vector<int64_t> first(n, -1);
        check(drm_dupset_mark(dups, ends.data(), (int64_t)n, (int64_t)item0, first.data()));
        auto dup = std::make_shared<std::vector<uint8_t>>(n * per, 0);
        for (size_t r = 0; r < n * per; ++r)
            (*dup)[r] = first[r / per] >= 0 && first[r / per] != (int64_t)(item0 + r / per);
        return dup;
    }

    // What the reference's sparse branch writes is only the SAM header: its write_sam_streaming call there
    // (post_processor.cpp:1004-1005) leaves out batch_query_count, which defaults to 0
    // (includes/utils/utils.hpp:99), so the row loop (utils.cpp:452) never runs. That header-only file is
    // the default here too (no rerank is computed for it). DRM_SAM_L2_ROWS=1 opts into the rows the
    // reranker meant to write: the L2 rows of every query, and none for a query whose
    // candidate range runs past the clipped expansion stream (the reference reads out of bounds there).
    // Both modes search the whole run first (faiss_search, src/main.cpp:278).
    int write_sparse_sam()
    {
        open_sam();
        const int rc = search(0, nq, &st);
        if (rc == DRM_OK && o.header_only)
            drm::write_sam_block(sam_block(0), 0, nullptr, k);
        else if (rc == DRM_OK)
            write_l2_rows();
        return rc;
    }

    // DRM_SAM_L2_ROWS=1 after the search of the whole run: the L2 rerank on the GRU window embeddings, then the blocks
    void write_l2_rows()
    {
        const auto tl = clk::now();
        drm_encoder *enc = nullptr;
        check(drm_encoder_load(o.model.c_str(), device, &enc));
        const int erc = drm_refs_embed(rt, enc, nullptr);
        drm_encoder_free(enc);
        check(erc);
        std::vector<float> l2d(nq * k);
        std::vector<uint64_t> l2i(nq * k);
        std::vector<int32_t> cnt(nq);
        int64_t bad = -1;
        const int lrc = drm_post_process_l2_dynamic(rt, I.p, (int64_t)nq, o.k_clusters, x.p, (int32_t)dim,
                                                    (int64_t)o.stride, o.k, o.k_clusters, l2d.data(), l2i.data(),
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
        std::cout << "[MAIN] L2 rerank (dynamic, stride " << o.stride << ") time: " << ms_since(tl) << " ms"
                  << std::endl;
        const size_t block = o.block(k);
        for (size_t lo = 0; lo < nq; lo += block) { // write_sam_streaming per reranked batch (:1004-1006)
            const size_t m = std::min(block, nq - lo);
            BlockAlignments ba;
            drm::SamAlignments av{};
            if (o.sam_cigar) {
                align_block(ba, l2i.data() + lo * k, cnt.data() + lo, lo, m, k);
                av = ba.view();
            }
            drm::SamBlock b = sam_block(lo);
            b.ids = l2i.data() + lo * k;
            b.aln = o.sam_cigar ? &av : nullptr;
            drm::write_sam_block(b, m, cnt.data() + lo, k);
        }
    }

    // The block loop of the streamed SAM modes over n items (reads, or pairs of `per` = 2 reads) in blocks of `block`:
    // per block the search + rerank of its reads, then produce(first item, items), which does the block's remaining GPU
    // work on this thread and returns the closure that writes its lines; that closure runs on a writer thread while the
    // next block is searched and produced, at most one writer alive at a time. A non-OK search ends the loop and is
    // returned; a throw from produce waits for the writer first; what a writer throws becomes DRM_ERR_IO at the end.
    template <class Produce> int stream_blocks(size_t n, size_t per, size_t block, Produce &&produce)
    {
        std::thread writer;
        std::string werr;
        auto join = [&] {
            if (writer.joinable())
                writer.join();
        };
        int rc = DRM_OK;
        for (size_t lo = 0; lo < n && rc == DRM_OK; lo += block) {
            const size_t m = std::min(block, n - lo);
            drm_search_stats bs{};
            rc = search(lo * per, m * per, &bs);
            st.nq += bs.nq;
            st.ndis += bs.ndis;
            st.nhops += bs.nhops;
            st.kernel_ms += bs.kernel_ms;
            std::function<void()> write;
            if (rc == DRM_OK) {
                try {
                    if (o.contigs)
                        contig_stage(lo * per, m * per);
                    const auto tp = clk::now();
                    write = produce(lo, m);
                    produce_ms += std::chrono::duration<double, std::milli>(clk::now() - tp).count();
                } catch (...) {
                    join();
                    throw;
                }
            }
            join();
            if (rc == DRM_OK && werr.empty())
                writer = std::thread([&werr, write] {
                    try {
                        write();
                    } catch (const std::exception &e) {
                        werr = e.what();
                    }
                });
        }
        join();
        if (rc == DRM_OK && !werr.empty())
            throw drm::Error(DRM_ERR_IO, werr);
        return rc;
    }

    // DRM_PAIR_RESCUE=1, the block of pairs res[] after drm_pair_hits: pair p's reads are queries lo + 2p and lo + 2p + 1.
    // A pair of status 1 gives two tasks (mate 2 against the insert window of mate 1's chosen hit, then mate 1 against
    // that of mate 2's), status 2 / 3 one; drm_mate_rescue scores them with the rerank's scoring and
    // drm_pair_rescue_choose decides. A rescued mate's window id goes where its chosen row's id would be in the list
    // handed to the aligner, and its pair counts as proper. `after` / `rescue_score` (DRM_SAM_MAPQ, null otherwise)
    // receive a rescued pair's record and the rescued mate's own score.
    void rescue_block(size_t lo, const std::vector<drm_pair_result> &res, std::vector<uint64_t> &chosen,
                      std::vector<int32_t> &cnt, std::vector<int32_t> &proper, std::vector<drm_pair_result> *after,
                      std::vector<int32_t> *rescue_score, std::vector<int32_t> *contig)
    {
        const size_t np = res.size();
        auto row_id = [&](size_t read, int32_t j) { return j >= 0 ? sw_ids.p[(lo + read) * k + (size_t)j] : (uint64_t)0; };
        auto row_score = [&](size_t read, int32_t j) { return j >= 0 ? sw_scores.p[(lo + read) * k + (size_t)j] : 0; };
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
        const drm_pair_params &prm = pair_prm;
        std::vector<drm_rescue_result> out(anchors.size());
        check(drm_mate_rescue(art, &rerank_scoring, &prm, anchors.data(), tq.data(), (int64_t)anchors.size(),
                              qbuf.p + lo * qs, ql.p + lo, (int32_t)qs, (int64_t)(2 * np), out.data()));
        for (size_t p = 0; p < np; ++p) {
            if (slot[2 * p] < 0 && slot[2 * p + 1] < 0)
                continue;
            const drm_rescue_result *rA = slot[2 * p] >= 0 ? &out[(size_t)slot[2 * p]] : nullptr;
            const drm_rescue_result *rB = slot[2 * p + 1] >= 0 ? &out[(size_t)slot[2 * p + 1]] : nullptr;
            if (o.contigs) {
                // the rescue guard: a rescued window that is not wholly inside its anchor's contig is no candidate
                auto guard = [&](const drm_rescue_result *&r, size_t anchor) {
                    if (!r || r->status != 0)
                        return;
                    uint64_t w = 0;
                    int32_t t = -1;
                    check(drm_mate_rescue_window(r, prm.ref_len, (int64_t)genome.size(), &w));
                    check(drm_contigs_find(ctg, (int64_t)(w >> 1), prm.ref_len, &t));
                    if (t < 0 || t != (*contig)[anchor])
                        r = nullptr;
                };
                guard(rA, 2 * p);
                guard(rB, 2 * p + 1);
                if (!rA && !rB)
                    continue;
            }
            drm_pair_result r{};
            uint64_t wr = 0;
            check(drm_pair_rescue_choose(&res[p], row_score(2 * p, res[p].j1), row_score(2 * p + 1, res[p].j2),
                                         row_id(2 * p, res[p].j1), row_id(2 * p + 1, res[p].j2), rA, rB, prm.ref_len,
                                         (int64_t)genome.size(), prm.unpaired_penalty, o.pair.rescue_min, &r, &wr));
            if (r.status != 5 && r.status != 6)
                continue;
            const size_t read = 2 * p + (r.status == 5 ? 1 : 0);
            chosen[read] = wr;
            cnt[read] = 1;
            if (contig)
                (*contig)[read] = (*contig)[read ^ 1]; // the guard: inside the anchor's contig
            proper[p] = 1;
            if (after) {
                (*after)[p] = r;
                (*rescue_score)[p] = (r.status == 5 ? rA : rB)->score;
            }
        }
    }

    // DRM_PAIR_TLEN=auto, before the block loop: the first min(pairs, DRM_PAIR_TLEN_SAMPLE) pairs are searched and
    // reranked as the block loop does it, drm_tlen_scan_device turns their rows (drm_search_rerank hands them over in
    // host memory, so they are uploaded once more) into the histogram of the confident pairs' template lengths, and
    // drm_tlen_estimate reads the window off its FR row into pair_prm. Fewer than kTlenMinSamples FR pairs: the default
    // 0,1000 stays. The rows are dropped: the block loop computes them again, so the file is that of the run with
    // DRM_PAIR_TLEN=<min>,<max> whatever DRM_SAM_BLOCK says.
    void estimate_tlen()
    {
        struct DeviceMem {
            void *p = nullptr;
            DeviceMem(const void *host, size_t bytes)
            {
                check(drm_malloc(&p, std::max<size_t>(bytes, 1)));
                if (host && bytes)
                    check(drm_memcpy_h2d(p, host, bytes));
            }
            ~DeviceMem() { drm_free(p); }
            DeviceMem(const DeviceMem &) = delete;
            DeviceMem &operator=(const DeviceMem &) = delete;
        };
        const size_t np = std::min(nq / 2, o.pair.tlen_sample), m = 2 * np;
        const int32_t ref_len = (int32_t)o.ref_len;
        const drm_tlen_params tp{o.pair.tlen_mapq, std::max(ref_len, 10000)};
        const size_t bins = (size_t)tp.max_scan + 1;
        std::vector<uint32_t> hist(3 * bins, 0);
        std::vector<drm_tlen_sample> samples(np);
        if (np) {
            drm_search_stats unused{};
            check(search(0, m, &unused));
            std::vector<int32_t> full(m);
            for (size_t r = 0; r < m; ++r)
                full[r] = untagged_length(qseqs[r]);
            check(drm_set_device(device));
            const DeviceMem d_ids(sw_ids.p, sizeof(uint64_t) * m * k), d_sc(sw_scores.p, sizeof(int32_t) * m * k),
                d_cnt(status.p, sizeof(int32_t) * m), d_full(full.data(), sizeof(int32_t) * m),
                d_hist(hist.data(), sizeof(uint32_t) * hist.size()), d_samples(nullptr, sizeof(drm_tlen_sample) * np);
            const uint64_t *ids = static_cast<const uint64_t *>(d_ids.p);
            const int32_t *sc = static_cast<const int32_t *>(d_sc.p), *cnt = static_cast<const int32_t *>(d_cnt.p),
                          *fl = static_cast<const int32_t *>(d_full.p);
            // DRM_CONTIGS: the contig stage chained on the device, the scan then reads its spread ids, scores and counts
            struct StageOut { // allocated under DRM_CONTIGS only
                DeviceMem ids, spread, sc, ctg, cnt;
                StageOut(size_t rows, size_t reads)
                    : ids(nullptr, sizeof(uint64_t) * rows), spread(nullptr, sizeof(uint64_t) * rows),
                      sc(nullptr, sizeof(int32_t) * rows), ctg(nullptr, sizeof(int32_t) * rows),
                      cnt(nullptr, sizeof(int32_t) * reads)
                {
                }
            };
            std::unique_ptr<StageOut> so;
            if (o.contigs) {
                so.reset(new StageOut(m * k, m));
                check(drm_contig_hits_device(ctg, ref_len, ids, sc, cnt, (int64_t)m, o.k,
                                             static_cast<uint64_t *>(so->ids.p), static_cast<uint64_t *>(so->spread.p),
                                             static_cast<int32_t *>(so->sc.p), static_cast<int32_t *>(so->ctg.p),
                                             static_cast<int32_t *>(so->cnt.p), nullptr));
                ids = static_cast<const uint64_t *>(so->spread.p);
                sc = static_cast<const int32_t *>(so->sc.p);
                cnt = static_cast<const int32_t *>(so->cnt.p);
            }
            check(drm_tlen_scan_device(&o.mapq_prm, &tp, ids, sc, cnt, ids + k, sc + k, cnt + 1, fl, fl + 1, (int64_t)np,
                                       o.k, 2, static_cast<drm_tlen_sample *>(d_samples.p),
                                       static_cast<uint32_t *>(d_hist.p), nullptr));
            check(drm_device_sync());
            check(drm_memcpy_d2h(hist.data(), d_hist.p, sizeof(uint32_t) * hist.size()));
            check(drm_memcpy_d2h(samples.data(), d_samples.p, sizeof(drm_tlen_sample) * np));
        }
        drm_tlen_estimate_t e{};
        check(drm_tlen_estimate(hist.data(), (int32_t)bins, kTlenMinSamples, &e));
        uint64_t cls[5] = {};
        for (const drm_tlen_sample &s : samples)
            ++cls[std::clamp(s.cls, 0, 4)];
        std::ostringstream classes;
        classes << "FR/RF/same/far = " << cls[1] << "/" << cls[2] << "/" << cls[3] << "/" << cls[4];
        if (e.status != 0) {
            std::cout << "[MAIN] Template length (auto): " << cls[1] << " FR pairs among " << np << " sampled, fewer than "
                      << kTlenMinSamples << ": falling back to min=" << pair_prm.min_tlen << " max=" << pair_prm.max_tlen
                      << "; " << classes.str() << std::endl;
        } else {
            // drm_mate_rescue scans dhi - dlo + ref_len rows, 2,048 at the most: the widest max_tlen it admits
            const int32_t widest = std::max(0, e.low - ref_len) + kRescueMaxRows;
            const bool cut = o.pair.rescue && e.high > widest;
            pair_prm.min_tlen = e.low;
            pair_prm.max_tlen = cut ? widest : e.high;
            std::cout << "[MAIN] Template length (auto): min=" << pair_prm.min_tlen << " max=" << pair_prm.max_tlen
                      << " mean=" << e.mean << " sd=" << e.sd << " from " << e.n << " of " << np << " pairs; "
                      << classes.str();
            if (cut)
                std::cout << " (max cut from " << e.high << " to the mate rescue's " << kRescueMaxRows << "-row cap)";
            std::cout << std::endl;
        }
        if (o.pair.rescue) {
            int64_t dlo = 0, dhi = 0;
            drm::check_rescue_params(&pair_prm, dlo, dhi);
        }
    }

    // One block of pairs [p0, p0 + mp), searched and reranked as 2 * mp interleaved reads: drm_pair_hits over the
    // block's lists (row_step 2), the alignment of only the chosen row of every read, and the two lines per pair.
    std::function<void()> produce_pairs(size_t p0, size_t mp)
    {
        const size_t lo = 2 * p0, m = 2 * mp, at = lo * k;
        auto ids = std::make_shared<std::vector<uint64_t>>(m, 0);
        auto cnt = std::make_shared<std::vector<int32_t>>(m, 0);
        auto proper = std::make_shared<std::vector<int32_t>>(mp, 0);
        auto line_mapq = std::make_shared<std::vector<int32_t>>(o.mapq ? m : 0, 0);
        auto ba = std::make_shared<BlockAlignments>();
        auto contig = std::make_shared<std::vector<int32_t>>(o.contigs ? m : 0, -1); // of each read's chosen row
        const uint64_t *lids = level_ids();
        std::vector<drm_pair_result> res(mp);
        check(drm_set_device(device));
        check(drm_pair_hits(&pair_prm, lids + at, sw_scores.p + at, status.p + lo, lids + at + k,
                            sw_scores.p + at + k, status.p + lo + 1, (int64_t)mp, o.k, 2, res.data()));
        for (size_t p = 0; p < mp; ++p) {
            const int32_t j[2] = {res[p].j1, res[p].j2};
            for (size_t t = 0; t < 2; ++t)
                if (j[t] >= 0) {
                    (*ids)[2 * p + t] = sw_ids.p[(lo + 2 * p + t) * k + (size_t)j[t]];
                    (*cnt)[2 * p + t] = 1;
                    if (o.contigs)
                        (*contig)[2 * p + t] = row_contig[(lo + 2 * p + t) * k + (size_t)j[t]];
                }
            (*proper)[p] = res[p].status == 0;
        }
        // DRM_SAM_MAPQ: the pair MAPQ of the same lists, before a rescue changes the choice
        std::vector<drm_pair_mapq_result> pm(o.mapq ? mp : 0);
        std::vector<int32_t> full(o.mapq ? m : 0), rescue_score(o.mapq ? mp : 0, 0);
        std::vector<drm_pair_result> after;
        if (o.mapq) {
            for (size_t r = 0; r < m; ++r)
                full[r] = untagged_length(qseqs[lo + r]);
            check(drm_pair_mapq(&pair_prm, &o.mapq_prm, lids + at, sw_scores.p + at, status.p + lo,
                                lids + at + k, sw_scores.p + at + k, status.p + lo + 1, full.data(), full.data() + 1,
                                res.data(), (int64_t)mp, o.k, 2, pm.data()));
            after = res;
        }
        if (o.pair.rescue)
            rescue_block(lo, res, *ids, *cnt, *proper, o.mapq ? &after : nullptr, o.mapq ? &rescue_score : nullptr,
                         o.contigs ? contig.get() : nullptr);
        if (o.mapq) {
            if (o.pair.rescue)
                check(drm_pair_mapq_rescued(&o.mapq_prm, after.data(), rescue_score.data(), full.data(), full.data() + 1,
                                            (int64_t)mp, 2, pm.data()));
            for (size_t p = 0; p < mp; ++p) {
                (*line_mapq)[2 * p] = pm[p].mapq1;
                (*line_mapq)[2 * p + 1] = pm[p].mapq2;
            }
        }
        align_block(*ba, ids->data(), cnt->data(), lo, m, 1, o.contigs ? contig->data() : nullptr);
        // DRM_SAM_DUP: one item per pair, a rescued mate keyed like any other mapped mate
        const auto dup = o.sam_dup ? mark_duplicates(*ba, ids->data(), cnt->data(), lo, p0, mp, 2, 1) : nullptr;
        // DRM_SAM_LOCI: the loci of every list whose chosen row j_m became the mate's line (not a rescued or unmapped
        // mate), head = j_m; the alternates, slots 1 .., are aligned in a pass of their own and printed as XA:Z
        const size_t na = o.loci ? (size_t)o.loci_prm.max_loci - 1 : 0;
        auto xa_ids = std::make_shared<std::vector<uint64_t>>(m * na, 0);
        auto xa_cnt = std::make_shared<std::vector<int32_t>>(na ? m : 0, 0);
        auto xa_contig = std::make_shared<std::vector<int32_t>>(o.contigs ? m * na : 0, -1);
        auto xa_ba = std::make_shared<BlockAlignments>();
        if (na) {
            std::vector<int32_t> head(m, -2); // -2: no row of the list, the "nothing" record
            for (size_t p = 0; p < mp; ++p) {
                const int32_t st = after[p].status;
                if (res[p].j1 >= 0 && st != 6)
                    head[2 * p] = res[p].j1;
                if (res[p].j2 >= 0 && st != 5)
                    head[2 * p + 1] = res[p].j2;
            }
            const BlockLoci b = hit_loci(lo, m, head);
            for (size_t r = 0; r < m; ++r)
                for (size_t j = 1; j < (size_t)b.n_loci[r]; ++j) {
                    const size_t row = (lo + r) * k + (size_t)b.rows[r * b.n + j];
                    (*xa_ids)[r * na + j - 1] = sw_ids.p[row];
                    if (o.contigs)
                        (*xa_contig)[r * na + j - 1] = row_contig[row];
                    (*xa_cnt)[r] = (int32_t)j;
                }
            align_block(*xa_ba, xa_ids->data(), xa_cnt->data(), lo, m, na, o.contigs ? xa_contig->data() : nullptr, false);
        }
        return [this, lo, mp, ids, cnt, proper, ba, line_mapq, contig, na, xa_ids, xa_cnt, xa_contig, xa_ba, dup] {
            const drm::SamContigs sc{&ctable, contig->data()}, xsc{&ctable, xa_contig->data()};
            const drm::SamAlignments xav = xa_ba->view();
            const drm::SamXa xa{xa_ids->data(), xa_cnt->data(), na, 0, &xav, o.contigs ? &xsc : nullptr};
            const drm::SamAlignments av = ba->view();
            drm::SamBlock b = sam_block(lo);
            b.ids = ids->data();
            b.aln = &av;
            b.mapq = o.mapq ? line_mapq->data() : nullptr;
            b.ctg = o.contigs ? &sc : nullptr;
            b.dup = dup ? dup->data() : nullptr;
            drm::write_sam_pairs(b, mp, cnt->data(), proper->data(), na ? &xa : nullptr);
        };
    }

    // DRM_SAM_LOCI: drm_hit_loci over the rerank rows of reads [lo, lo + m) with the given head rows, on the spread ids
    // under DRM_CONTIGS; a slot's real id and contig are those of its row (loci_rows) in the rerank's arrays
    struct BlockLoci {
        size_t n = 0; // slots per read
        std::vector<drm_mapq_result> rec;
        std::vector<int32_t> n_loci, n_pass, scores, rows, size;
        std::vector<uint64_t> ids;
    };
    BlockLoci hit_loci(size_t lo, size_t m, const std::vector<int32_t> &head)
    {
        BlockLoci b;
        b.n = (size_t)o.loci_prm.max_loci;
        b.rec.resize(m);
        b.n_loci.resize(m);
        b.n_pass.resize(m);
        b.ids.resize(m * b.n);
        b.scores.resize(m * b.n);
        b.rows.resize(m * b.n);
        b.size.resize(m * b.n);
        std::vector<int32_t> full(m);
        for (size_t i = 0; i < m; ++i)
            full[i] = untagged_length(qseqs[lo + i]);
        check(drm_set_device(device));
        check(drm_hit_loci(&o.mapq_prm, &o.loci_prm, level_ids() + lo * k, sw_scores.p + lo * k, status.p + lo,
                           head.data(), full.data(), (int64_t)m, o.k, b.rec.data(), b.n_loci.data(), b.n_pass.data(),
                           b.ids.data(), b.scores.data(), b.rows.data(), b.size.data()));
        return b;
    }

    // DRM_SAM_LOCI, single reads: one drm_hit_loci per block with head = row 0 (the primary, as DRM_SAM_MAPQ has it),
    // the alignment of only the recorded loci's head rows (width n), and per read its primary line from slot 0 and a
    // secondary line -- or with DRM_SAM_XA an XA:Z entry -- per further slot. A read without a head, or whose best
    // score is below min_score, keeps no row and is written unmapped.
    std::function<void()> produce_loci(size_t lo, size_t m)
    {
        const BlockLoci b = hit_loci(lo, m, std::vector<int32_t>(m, 0));
        const size_t n = b.n;
        auto ids = std::make_shared<std::vector<uint64_t>>(m * n, 0);
        auto cnt = std::make_shared<std::vector<int32_t>>(m, 0);
        auto contig = std::make_shared<std::vector<int32_t>>(o.contigs ? m * n : 0, -1);
        auto line_mapq = std::make_shared<std::vector<int32_t>>(m * n, 0); // secondary lines print 0
        auto ba = std::make_shared<BlockAlignments>();
        for (size_t i = 0; i < m; ++i) {
            if (b.rec[i].status != 0 || b.rec[i].best_score < o.mapq_prm.min_score)
                continue;
            (*cnt)[i] = b.n_loci[i];
            (*line_mapq)[i * n] = b.rec[i].mapq;
            for (size_t j = 0; j < (size_t)b.n_loci[i]; ++j) {
                const size_t row = (lo + i) * k + (size_t)b.rows[i * n + j];
                (*ids)[i * n + j] = sw_ids.p[row];
                if (o.contigs)
                    (*contig)[i * n + j] = row_contig[row];
            }
        }
        align_block(*ba, ids->data(), cnt->data(), lo, m, n, o.contigs ? contig->data() : nullptr);
        // DRM_SAM_DUP: one item per read, keyed by its primary locus (slot 0)
        const auto dup = o.sam_dup ? mark_duplicates(*ba, ids->data(), cnt->data(), lo, lo, m, 1, n) : nullptr;
        return [this, lo, m, n, ids, cnt, contig, ba, line_mapq, dup] {
            const drm::SamAlignments av = ba->view();
            const drm::SamContigs sc{&ctable, contig->data()};
            drm::SamBlock b = sam_block(lo);
            b.ids = ids->data();
            b.aln = &av;
            b.mapq = line_mapq->data();
            b.ctg = o.contigs ? &sc : nullptr;
            b.dup = dup ? dup->data() : nullptr;
            drm::write_sam_block(b, m, cnt->data(), n, /*loci=*/true, o.sam_xa);
        };
    }

    // One block of reads [lo, lo + m): its rows (the search's, or the rerank's), and with DRM_SAM_CIGAR their
    // alignments (post_process_*_dynamic_streaming + write_sam_streaming, src/main.cpp:316-319,
    // src/utils/utils.cpp:409-503)
    std::function<void()> produce_reads(size_t lo, size_t m)
    {
        if (o.loci)
            return produce_loci(lo, m);
        const bool from_search = o.sam_from_search;
        const size_t kr = from_search ? kc : k;
        const uint64_t *rows = from_search ? reinterpret_cast<const uint64_t *>(I.p) + lo * kc : sw_ids.p + lo * k;
        auto cnt = std::make_shared<std::vector<int32_t>>(m);
        auto line_mapq = std::make_shared<std::vector<int32_t>>(o.mapq ? m * kr : 0, 0);
        auto ba = std::make_shared<BlockAlignments>();
        for (size_t i = 0; i < m; ++i)
            (*cnt)[i] = from_search ? std::min(o.k, o.k_clusters) : std::max(status.p[lo + i], 0);
        if (o.sam_cigar) {
            if (o.mapq) { // DRM_SAM_MAPQ: the locus scan of the block's rerank rows, head = the primary row
                std::vector<int32_t> full(m), head(m, 0);
                std::vector<drm_mapq_result> res(m);
                for (size_t i = 0; i < m; ++i)
                    full[i] = untagged_length(qseqs[lo + i]);
                check(drm_set_device(device));
                const uint64_t *lids = o.contigs ? spread.data() + lo * k : rows; // DRM_CONTIGS: the spread ids
                check(drm_hit_mapq(&o.mapq_prm, lids, sw_scores.p + lo * k, status.p + lo, head.data(), full.data(),
                                   (int64_t)m, o.k, res.data()));
                for (size_t i = 0; i < m; ++i)
                    (*line_mapq)[i * kr] = res[i].mapq; // secondary lines print 0
            }
            align_block(*ba, rows, cnt->data(), lo, m, kr, o.contigs ? row_contig.data() + lo * k : nullptr);
        }
        return [this, lo, m, kr, rows, cnt, ba, line_mapq] {
            const drm::SamAlignments av = ba->view();
            const drm::SamContigs sc{&ctable, o.contigs ? row_contig.data() + lo * k : nullptr};
            drm::SamBlock b = sam_block(lo);
            b.ids = rows;
            b.aln = o.sam_cigar ? &av : nullptr;
            b.mapq = o.mapq ? line_mapq->data() : nullptr;
            b.ctg = o.contigs ? &sc : nullptr;
            drm::write_sam_block(b, m, cnt->data(), kr);
        };
    }

    // DRM_SAM_SORT=coordinate, after the last block: one drm_sort_order over the keys of every spooled line, then the
    // header and the lines in that order. Equal keys keep the order of the unsorted file, so the result does not depend
    // on DRM_SAM_BLOCK.
    void write_sorted_sam()
    {
        const size_t n = spool.keys.size();
        std::vector<uint32_t> order(n);
        auto t0 = clk::now();
        check(drm_sort_order(spool.keys.data(), (int64_t)n, device, order.data()));
        const double sort_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
        t0 = clk::now();
        const drm::SamContigs sc{&ctable, nullptr};
        drm::SamBlock b = sam_block(0);
        b.ctg = o.contigs ? &sc : nullptr;
        if (o.sam_bam)
            drm::write_bam_sorted(b, spool, order.data());
        else
            drm::write_sam_sorted(b, spool, order.data());
        if (o.sam_stats)
            std::cout << "[MAIN] SAM sort: " << n << " lines, " << sort_ms << " ms for the order (copies included), "
                      << std::chrono::duration<double, std::milli>(clk::now() - t0).count()
                      << " ms for the final write" << std::endl;
    }

    // the search + rerank and, with use_streaming, the SAM of the chosen output mode; returns the search's code
    int run()
    {
        art = rt;
        if (o.sam_cigar && !art)
            art = genome_handle();
        if (o.stream_sam && k > kc * 2 * o.stride) // post_processor.cpp:769-772
            throw drm::Error(DRM_ERR_K, "Final k too large. Ensure k < k_clusters * 2 * stride to have enough candidates.");
        if (o.l2_rows_from_sw)
            std::cout << "[MAIN] stride > 1 without the GRU model on one device: SAM rows from the SW rerank (the "
                         "reference reranks them by L2 here)"
                      << std::endl;
        if (o.header_only || o.l2_rows)
            return write_sparse_sam();
        if (!o.stream_sam)
            return search(0, nq, &st);
        if (o.paired && o.pair.tlen_auto)
            estimate_tlen();
        if (o.sam_dup) // after the estimate's sample run: the set sees the block loop's items only
            check(drm_dupset_create((int64_t)std::max<size_t>(o.paired ? nq / 2 : nq, 1), device, &dups));
        open_sam(o.paired ? " (paired)" : "");
        const auto t0 = clk::now();
        const int rc =
            o.paired // DRM_SAM_BLOCK counts pairs here; the file does not depend on it
                ? stream_blocks(nq / 2, 2, o.block(2), [&](size_t p0, size_t mp) { return produce_pairs(p0, mp); })
                // blocks of DRM_SAM_BLOCK queries; the file does not depend on it
                : stream_blocks(nq, 1, o.block(o.sam_from_search ? (size_t)std::min(o.k, o.k_clusters) : k),
                                [&](size_t lo, size_t m) { return produce_reads(lo, m); });
        if (o.sam_stats)
            std::cout << "[MAIN] SAM stage: " << produce_ms << " ms between the rerank and the writer, " << aligned_rows
                      << " rows aligned, " << std::chrono::duration<double, std::milli>(clk::now() - t0).count()
                      << " ms for the block loop" << std::endl;
        if (rc == DRM_OK && o.sam_sort)
            write_sorted_sam();
        else if (rc == DRM_OK && o.sam_bam) // after the last block: the remainder and the EOF member
            bam.finish();
        if (rc == DRM_OK && o.sam_bam && o.sam_stats)
            std::cout << "[MAIN] BAM compression: " << bam.bytes_in << " bytes in, " << bam.bytes_out << " bytes out, "
                      << bam.compress_ms << " ms in drm_bgzf_compress" << std::endl;
        return rc;
    }

    // save_results (src/utils/utils.cpp:264-334)
    void save()
    {
        if (!o.is_npy) // rows of a query with no candidate at all (reranker.cpp:10-11) stay -1 / 2^64-1
            for (size_t i = 0; i < nq; ++i)
                for (size_t j = (size_t)std::max(status.p[i], 0); j < k; ++j) {
                    sw_scores.p[i * k + j] = -1;
                    sw_ids.p[i * k + j] = ~0ull;
                }
        const auto t0 = clk::now();
        std::filesystem::create_directories(o.out_dir);
        const size_t kout = o.stride == 1 ? k : kc;
        std::vector<uint64_t> idx(nq * kout);
        std::vector<float> dis(nq * kout);
        for (size_t i = 0; i < nq; ++i)
            for (size_t j = 0; j < kout; ++j) {
                idx[i * kout + j] = (uint64_t)I.p[i * kc + j];
                dis[i * kout + j] = D.p[i * kc + j];
            }
        drm::npy_save(o.out_dir + "/indices.npy", idx.data(), {nq, kout}, 'u', 8);
        drm::npy_save(o.out_dir + "/distances.npy", dis.data(), {nq, kout}, 'f', 4);
        if (!o.is_npy) {
            drm::npy_save(o.out_dir + "/sw_scores.npy", sw_scores.p, {nq, k}, 'i', 4);
            drm::npy_save(o.out_dir + "/sw_ids.npy", sw_ids.p, {nq, k}, 'u', 8);
        }
        std::cout << "[MAIN] Output saving time: " << ms_since(t0) << " ms" << std::endl;
    }
};

int main(int argc, char *argv[])
{
    if (argc < 4 || argc > 10) {
        std::cerr << "Usage: " << argv[0]
                  << " <index_prefix> <query_seqs.fastq> <ref_seqs.fasta> [EF] [K] [K_clusters] [output_dir] "
                     "[use_dynamic] [use_streaming]\n"
                     "  - query input: Can be FASTQ/FASTA/TXT file or pre-computed embeddings in .npy format\n"
                     "  - EF: Optional HNSW search parameter (default: 128)\n"
                     "  - K: Optional number of nearest neighbors to return (default: 128)\n"
                     "  - output_dir: Optional output directory (default: current directory)"
                  << std::endl;
        return 1;
    }
    try {
        auto master = clk::now();
        std::cout << "=== DeepReadMapper MI355X Pipeline ===" << std::endl << std::endl;
        const std::string prefix = argv[1];
        const std::string base = std::filesystem::path(prefix).filename().string();
        const std::string config_file = prefix + "/config.txt";
        if (!std::filesystem::exists(config_file))
            throw drm::Error(DRM_ERR_IO, "Config file does not exist: " + config_file);
        auto config = drm::load_config(config_file);
        if (!config.count("ref_len") || !std::holds_alternative<size_t>(config["ref_len"]) || !config.count("stride") ||
            !std::holds_alternative<size_t>(config["stride"]))
            throw drm::Error(DRM_ERR_FORMAT, "config.txt lacks integer ref_len / stride");
        const Options o =
            read_options(argc, argv, std::get<size_t>(config["ref_len"]), std::get<size_t>(config["stride"]));

        Pipeline p(o);
        auto t0 = clk::now();
        if (!p.load_queries())
            return 1;
        p.load_reference();
        std::cout << "[MAIN] Total Data loading time: " << ms_since(t0) << " ms" << std::endl << std::endl;
        p.open(prefix + "/" + base + ".index");
        p.embed();
        p.alloc_buffers();

        t0 = clk::now();
        const int rc = p.run();
        const std::string err = rc == DRM_OK ? "" : drm_last_error();
        const long search_ms = ms_since(t0);
        if (p.art != p.rt)
            drm_refs_free(p.art);
        drm_contigs_free(p.ctg);
        drm_dupset_free(p.dups);
        drm_refs_free(p.rt); // the free calls take null
        drm_index_free(p.index);
        drm_multi_free(p.multi);
        if (rc != DRM_OK)
            throw drm::Error(rc, err);
        std::cout << "[MAIN] Search" << (o.is_npy ? "" : " + SW rerank") << " time: " << search_ms << " ms (device "
                  << p.st.kernel_ms << " ms, ndis " << p.st.ndis << ", nhops " << p.st.nhops << ", " << o.devices.size()
                  << " device(s))" << std::endl;

        // outputs; skipped with use_streaming (src/main.cpp:371, :409-412)
        if (o.use_streaming)
            std::cout << "[MAIN] Skip normal output saving since streaming output is used." << std::endl;
        else
            p.save();
        std::cout << "[MAIN] Total pipeline time: " << ms_since(master) << " ms" << std::endl;
        std::cout << "=== Pipeline Completed Successfully! ===" << std::endl;
    } catch (const std::exception &e) {
        std::cerr << "Error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
