// deepreadmapper_amd/csrc/drm_internal.h -- private C++ API shared by the library and the CLIs.
#pragma once
#include <cstdint>
#include <new>
#include <stdexcept>
#include <string>
#include <string_view>
#include <unordered_map>
#include <variant>
#include <vector>

#include "drm_hip.h"

namespace drm {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

void set_last_error(const std::string &msg);

// The body of an extern "C" entry point: runs f and turns what it throws into the call's return code and
// drm_last_error's message. An Error gives its own code; anything else gives `other`.
template <class F> int guarded(F &&f, int other = DRM_ERR_ARG)
{
    try {
        f();
        return DRM_OK;
    } catch (const Error &e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        set_last_error("out of host memory");
        return other;
    } catch (const std::exception &e) {
        set_last_error(e.what());
        return other;
    }
}

// RCCL helpers over a drm_comm (exec.cpp), for collectives the C ABI builds on (drm_index_broadcast, capi.cpp):
// a grouped ncclBroadcast of byte ranges from `root` (send is read on the root only; recv may equal send there),
// synchronised on `stream`; and an agreement step (min over ranks of `ok`) that every rank reaches before a
// collective that a failed rank would not enter
struct BcastItem {
    const void *send;
    void *recv;
    size_t bytes;
};
int comm_rank(const drm_comm *c);
int comm_nranks(const drm_comm *c);
int comm_device(const drm_comm *c);
void comm_broadcast(drm_comm *c, const BcastItem *items, int n, int root, void *stream); // throws Error
int comm_all_ok(drm_comm *c, bool ok, void *stream);                                   // throws Error

// ---------------------------------------------------------------------------------------------
// Host image of a faiss IndexHNSWPQ: exactly the fields faiss::write_index / read_index touch
// for fourcc "IHNp" + storage "IxPq" [faiss impl/index_write.cpp, impl/index_read.cpp].
// ---------------------------------------------------------------------------------------------
struct IndexHeader {
    int32_t d = 0;
    int64_t ntotal = 0;
    uint8_t is_trained = 1;
    int32_t metric_type = 1; // METRIC_L2
    float metric_arg = 0.f;
};

struct HnswPqHost {
    IndexHeader hdr;
    // faiss::HNSW
    std::vector<double> assign_probas;
    std::vector<int32_t> cum_nneighbor_per_level;
    std::vector<int32_t> levels;   // level + 1 per node
    std::vector<uint64_t> offsets; // ntotal + 1
    std::vector<int32_t> neighbors;
    int32_t entry_point = -1;
    int32_t max_level = -1;
    int32_t efConstruction = 40;
    int32_t efSearch = 16;
    int32_t upper_beam = 1;
    // storage: faiss::IndexPQ
    IndexHeader storage_hdr;
    uint64_t pq_d = 0, pq_M = 0, pq_nbits = 0;
    std::vector<float> centroids; // [M][ksub][dsub]
    std::vector<uint8_t> codes;   // [ntotal][code_size]
    int32_t search_type = 0;
    uint8_t encode_signs = 0;
    int32_t polysemous_ht = 0;

    int dsub() const { return pq_M ? int(pq_d / pq_M) : 0; }
    int ksub() const { return 1 << int(pq_nbits); }
    int code_size() const { return int((pq_M * pq_nbits + 7) / 8); }
    int deg0() const { return cum_nneighbor_per_level.size() > 1 ? cum_nneighbor_per_level[1] - cum_nneighbor_per_level[0] : 0; }
    int nb_at(int level) const { return cum_nneighbor_per_level[level + 1] - cum_nneighbor_per_level[level]; }
};

HnswPqHost read_hnswpq(const std::string &path);                 // throws Error
void write_hnswpq(const HnswPqHost &ix, const std::string &path); // throws Error
void validate_hnswpq(const HnswPqHost &ix);                      // throws Error(DRM_ERR_FORMAT)

// ---------------------------------------------------------------------------------------------
// Host image of an hnswlib HierarchicalNSW<float> file (saveIndex/loadIndex, hnswlib_io.cpp):
// the reference's fp32-L2 backend (src/hnswlib_dir/*).
// ---------------------------------------------------------------------------------------------
struct HnswFlatHost {
    int32_t d = 0;
    int64_t n = 0;
    uint64_t max_elements = 0, maxM = 0, maxM0 = 0, M = 0, efc = 0;
    int32_t maxlevel = -1;
    uint32_t ep = 0;
    double mult = 0.0;
    std::vector<float> vec;       // [n][d]
    std::vector<uint32_t> l0;     // [n][1 + maxM0]: header (count in low 16 bits), links
    std::vector<uint64_t> labels; // [n]
    std::vector<int32_t> levels;  // [n]
    std::vector<int64_t> up_off;  // [n]: first word of the node's upper blocks in `up`, -1 if none
    std::vector<uint32_t> up;     // blocks of (1 + maxM) words, block l-1 = level l
};
HnswFlatHost read_hnswlib(const std::string &path);                  // throws Error
void write_hnswlib(const HnswFlatHost &ix, const std::string &path); // throws Error
void build_hnsw_flat(const float *x, int64_t n, int d, int M, int efc, int nthreads, uint64_t seed,
                     const std::string &path);

// faiss HNSW::set_default_probas(M, 1/log(M)) [faiss impl/HNSW.cpp]
void hnsw_default_probas(int M, std::vector<double> &probas, std::vector<int32_t> &cum);

// ---------------------------------------------------------------------------------------------
// Formats (src/utils/utils.cpp, src/utils/parse_inputs.cpp)
// ---------------------------------------------------------------------------------------------
using ConfigValue = std::variant<size_t, float, std::string>; // includes/utils/utils.hpp:102

void save_config(const std::unordered_map<std::string, ConfigValue> &config, const std::string &folder,
                 const std::string &file = "config.txt");
std::unordered_map<std::string, ConfigValue> load_config(const std::string &path);

// cnpy-compatible npy v1.0 writer/reader (descr '<u8', '<f4', '<i4', ...)
void npy_save(const std::string &path, const void *data, const std::vector<size_t> &shape, char kind, int itemsize);
struct NpyArray {
    std::vector<size_t> shape;
    char kind = 'f';
    int itemsize = 4;
    bool fortran = false;
    std::vector<uint8_t> bytes;
};
NpyArray npy_load(const std::string &path);

std::string reverse_complement(const std::string &seq);
// format_fasta (parse_inputs.cpp:223-369): fwd/RC interleaved windows; lookup_mode=false adds "<" ">".
std::vector<std::string> format_fasta(const std::string &data, size_t ref_len, size_t stride, bool lookup_mode);
// format_fastq (parse_inputs.cpp:843-950): "<"+seq+">" and ids up to ' ', '\t', '/'.
void format_fastq(const std::string &data, std::vector<std::string> &seqs, std::vector<std::string> &ids);
// format_fastq that also keeps each record's fourth line (DRM_SAM_QUAL; no reference counterpart: the reference drops
// it). Throws Error(DRM_ERR_FORMAT) naming the read when a quality line's length differs from its read's.
void format_fastq_qual(const std::string &data, std::vector<std::string> &seqs, std::vector<std::string> &ids,
                       std::vector<std::string> &quals);
// read_file (utils.cpp:188-215) dispatch on extension; .txt = one sequence per non-empty line.
void read_file(const std::string &path, std::vector<std::string> &seqs, std::vector<std::string> &ids,
               size_t ref_len = 150, size_t stride = 1, bool lookup_mode = false);
// read_file for a query file, with the quality lines of a .fastq / .fq (format_fastq_qual); any other format leaves
// quals empty.
void read_file_qual(const std::string &path, std::vector<std::string> &seqs, std::vector<std::string> &ids,
                    std::vector<std::string> &quals);
std::string read_whole_file(const std::string &path);
// extract_FASTA_sequence (parse_inputs.cpp:174-220): skip the first line, keep the upper-cased
// A/C/G/T/N letters of everything after it (later header lines included), drop the rest.
std::string extract_fasta_sequence(const std::string &path);
// The contigs of a FASTA in the coordinates of extract_fasta_sequence's string (include/drm_hip.h,
// drm_fasta_contigs); throws Error(DRM_ERR_FORMAT) naming the contig.
struct FastaContig {
    std::string name;
    int64_t start = 0, len = 0;
};
std::vector<FastaContig> fasta_contigs(const std::string &path);
// ---------------------------------------------------------------------------------------------
// SAM (sam.cpp): write_sam / write_sam_streaming (utils.cpp:336-503), one block of queries per call
// ---------------------------------------------------------------------------------------------
// The GPU alignment of every row of a block (the DRM_SAM_CIGAR mode, no reference counterpart: the reference's CIGAR
// is a TODO). A row with a record is written with its real leftmost POS, soft clips, SEQ reverse-complemented and QUAL
// reversed under flag 16, and the tags AS:i:<score> NM:i:<nm>; a status-1 record is written unmapped (FLAG | 4, POS 0,
// CIGAR *, MAPQ 0, no tags).
struct SamAlignments {
    const drm_sw_alignment *rec; // drm_sw_align of the row's window with its tagged query
    const uint32_t *ops;         // row r's complete operations start at ops + ops_off[r]
    const int64_t *ops_off;
    // DRM_SAM_SCORING / DRM_SAM_FLANK (drm_sw_align_affine over the row's flanked region, drm_sw_align_region): the
    // record is relative to genome[region_start[r] ..+ region_len[r]) and the row is formatted by drm_sam_cigar_region's
    // rules; AS is then the affine score. Null: the window of the row's id (drm_sam_cigar).
    const int64_t *region_start = nullptr;
    const int32_t *region_len = nullptr;
    // DRM_SAM_MD (drm_sw_align_md of the same rows): every mapped line gets MD:Z:<drm_sam_md of the row> behind NM:i;
    // row r has the record md[r] and its complete words at md_words + md_off[r]
    const drm_sw_md *md = nullptr;
    const uint32_t *md_words = nullptr;
    const int64_t *md_off = nullptr;
};
// DRM_CONTIGS: the contig table of the reference and the contig of every row. The header then holds one @SQ line per
// contig in file order (SN its name, LN its length), a row's RNAME is its contig's name and its POS counts from the
// contig's start.
struct SamContigs {
    const std::vector<FastaContig> *table;
    const int32_t *row_contig; // indexed like the rows' ids
};
// What both writers need to know about a block. Row r of the block is one (query, window) pair: ids[r] its dense
// window id, aln->rec[r] its alignment, mapq[r] its MAPQ, ctg->row_contig[r] its contig.
struct SamBlock {
    std::string path;
    bool header = false;          // true: truncate and write @HD / @SQ first; false: append
    std::string ref_name = "ref"; // @SQ SN / RNAME without contigs; LN is ref_len (the reference's quirk)
    size_t ref_len = 0;           // the window length
    const std::vector<std::string> *queries = nullptr;   // every query of the run, tagged ("<" read ">") or not
    const std::vector<std::string> *query_ids = nullptr; // QNAME; a missing or empty one prints S1/<number>/0
    // DRM_SAM_QUAL (null or empty = "*" in column 11): the quality line of every query, indexed like queries; printed
    // reversed on a line whose SEQ is printed reverse-complemented
    const std::vector<std::string> *quals = nullptr;
    size_t q0 = 0;                      // the block's first query
    const uint64_t *ids = nullptr;      // [rows]
    const SamAlignments *aln = nullptr; // null (write_sam_block only): the reference's pseudo fields
    const int32_t *mapq = nullptr;      // DRM_SAM_MAPQ (null = "60" on every line); a row written unmapped prints 0
    const SamContigs *ctg = nullptr;    // with aln only; null = the one sequence ref_name
    // DRM_SAM_DUP (null = no line is marked): per query of the block, indexed from q0; a query with dup != 0 has 1024
    // added to the flag of every line it prints (primary, secondary, unmapped); XA entries are untouched
    const uint8_t *dup = nullptr;
    // DRM_SAM_SORT=coordinate (null = the lines go to the file): the writers touch no file; every line they build is
    // appended to the spool instead, in the order in which it would have been written
    struct SamSpool *spool = nullptr;
    // DRM_SAM_FORMAT=bam (null = SAM text): every line is encoded as a BAM alignment record (bam_encode_line). Without
    // a spool the records go to this sink, which the first block (header) opens on `path`; with a spool they are what
    // the spool holds in place of text
    class BamSink *bam = nullptr;
};
// The lines of a run held back until their order is known: line i is text[offsets[i] .. offsets[i + 1]) (the last one
// to the end), newline included, and keys[i] its drm_sam_sort_key. All of it lives in host memory, a few hundred bytes
// per line; a run whose lines do not fit needs an external merge, which this does not do.
struct SamSpool {
    std::string text;
    std::vector<uint64_t> offsets, keys;
};
// The sorted file: @HD VN:1.0 SO:coordinate, b's @SQ lines (path, ref_name, ref_len and ctg->table are read), then line
// order[i] of the spool for i = 0 .. The file is written beside b.path and renamed over it when complete.
void write_sam_sorted(const SamBlock &b, const SamSpool &spool, const uint32_t *order);

// The eleven columns of one line and its tags. `reversed` is the orientation of columns 10 and 11: SEQ
// reverse-complemented and QUAL reversed, or both as read. An empty read or quality line prints "*".
struct SamLine {
    std::string_view qname;
    int flag = 0;
    std::string_view rname = "*";
    int64_t pos = 0;
    int mapq = 0;
    std::string_view cigar = "*", rnext = "*";
    int64_t pnext = 0, tlen = 0;
    std::string_view read, qual;
    bool reversed = false;
    std::string tags; // "\tAS:i:..\tNM:i:..[\tMD:Z:..][\tXA:Z:..]" of a mapped row, else empty
};
// The index of every reference name among the @SQ lines
using SamRefIds = std::unordered_map<std::string_view, int64_t>;
// Appends the BAM alignment record of one line (SAMv1 sec. 4.2, block_size first; include/drm_hip.h, drm_bam_record, has
// the rules and the errors). The one encoder: drm_bam_record parses its text into a SamLine and calls this, and the
// writers call it with the line they built.
void bam_encode_line(const SamLine &l, const SamRefIds &refs, std::string &out);
// "BAM\1", l_text, the text, n_ref and per @SQ line of the text l_name, name, NUL, l_ref (drm_bam_header)
void bam_encode_header(std::string_view text, std::string &out);

// the input bytes of one BGZF block (htslib's BGZF_BLOCK_SIZE); drm_bgzf_block
constexpr int kBgzfBlock = 65280;
// DRM_SAM_FORMAT=bam: where the writers of sam.cpp send a run's BAM bytes. They know this interface alone, so that
// sam.cpp stands without the encoder and the compressor behind it: encode() appends one line's record, begin() opens the
// file and takes the header, records are appended to pending() and flush() is called behind each, finish() ends the file.
class BamSink {
public:
    virtual ~BamSink() = default;
    virtual void encode(const SamLine &l, const SamRefIds &refs, std::string &to) = 0;
    virtual void begin(const std::string &path, std::string_view header_text) = 0;
    virtual std::string &pending() = 0;
    virtual void flush(bool all = false) = 0;
    virtual void finish() = 0;
};
// The sink of bin/pipeline (bam.cpp): encode() is bam_encode_line; the bytes are compressed by drm_bgzf_compress on
// `device` in whole multiples of the 65,280-byte BGZF block whenever about 4 MiB have come together, the tail is carried
// on, and finish() compresses what is left and adds the empty EOF member. The file is therefore a function of the byte
// stream alone, whatever blocks the stream arrived in.
class BamFile : public BamSink {
public:
    int device = 0;
    uint64_t bytes_in = 0, bytes_out = 0; // DRM_SAM_STATS: what went into the compression and what came out
    double compress_ms = 0;              // and the time inside drm_bgzf_compress
    void encode(const SamLine &l, const SamRefIds &refs, std::string &to) override;
    void begin(const std::string &path, std::string_view header_text) override;
    std::string &pending() override { return buf; }
    void flush(bool all = false) override;
    void finish() override; // throws Error(DRM_ERR_IO) when the file did not take it all
    ~BamFile() override;

private:
    std::string buf, file_path;
    std::vector<uint8_t> packed;
    void *file = nullptr; // a FILE *
};
// The sorted BAM file, write_sam_sorted's twin: the header under SO:coordinate, then record order[i] of the spool (whose
// text holds encoded records) for i = 0 .., through b.bam onto b.path + ".part", renamed over b.path when complete.
void write_bam_sorted(const SamBlock &b, const SamSpool &spool, const uint32_t *order);
// The SAM lines of queries [q0, q0 + nq): query i has the rows i * k + j, j < counts[i]; row 0 is the primary, later
// rows secondaries (flag 256). Without alignments a row prints the reference's pseudo fields
//   QNAME FLAG ref <window's start + 1> 60 <read length>M * 0 0 SEQ QUAL       (SEQ and QUAL as read, also under flag 16)
// `loci` (DRM_SAM_LOCI, with aln only): the rows of a query are its distinct loci (drm_hit_loci's slots, k = max_loci).
// Under `loci` or contigs a query without rows is written as one unmapped line (flag 4). With `xa` (DRM_SAM_XA) rows
// 1 .. get no line of their own: the primary line ends in the tag
//   XA:Z:<RNAME>,<+|-><POS>,<CIGAR>,<NM>;...
// one entry per such row that holds an alignment, POS 1-based in the contig's own coordinates, the sign the strand,
// the CIGAR drm_sam_cigar's (drm_sam_cigar_region's over a flanked region); no tag when no entry remains.
void write_sam_block(const SamBlock &b, size_t nq, const int32_t *counts, size_t k, bool loci = false,
                     bool xa = false);
// The alternates behind an XA:Z tag: those of block row r are ids[r * width + j] for first <= j < counts[r], with their
// alignments aln->rec[r * width + j] and, under DRM_CONTIGS, their contigs ctg->row_contig[r * width + j].
struct SamXa {
    const uint64_t *ids;
    const int32_t *counts;
    size_t width, first;
    const SamAlignments *aln;
    const SamContigs *ctg;
};
// The paired form (DRM_MATES, no reference counterpart): the two primary lines of pairs whose reads are queries
// q0 + 2 * p (mate 1) and q0 + 2 * p + 1 (mate 2). Row r = 2 * p + m of the block carries the read's chosen window
// (counts[r] = 1, or 0 for a read without a hit) and its alignment as in write_sam_block (b.aln is required); a read
// without a hit or with a status-1 record is unmapped. proper[p] != 0: drm_pair_hits chose a proper combination. The
// fields that relate the two lines are drm_sam_pair_fields' (include/drm_hip.h):
//   mapped:   QNAME FLAG ref POS 60 CIGAR = PNEXT TLEN SEQ * AS:i:<score> NM:i:<nm>
//   unmapped: QNAME FLAG ref|* POS 60 * =|* PNEXT TLEN SEQ *        (SEQ as read; "*" when neither mate is mapped)
// Under contigs an unmapped mate takes its mate's RNAME and POS; mates on one contig print RNEXT "=", mates on two the
// other's name and local PNEXT, TLEN 0 and never flag 0x2.
// `xa` (DRM_SAM_LOCI, null = no tag): the alternates of row r; a mapped mate's line ends in their XA:Z tag, and nothing
// else on the line changes.
void write_sam_pairs(const SamBlock &b, size_t npairs, const int32_t *counts, const int32_t *proper,
                     const SamXa *xa = nullptr);

#if defined(__HIPCC__)
#define DRM_HOST_DEVICE __host__ __device__
#else
#define DRM_HOST_DEVICE
#endif
// genome[start, start + len), read backwards and complemented when `reverse`; len 0 = no region
struct GenomeRegion {
    int64_t start;
    int32_t len, reverse;
};
// The printed alignment (include/drm_hip.h, drm_sw_align_region): the region of one window id, its window widened by
// `flank` bases on either side and clamped to the genome; none for a window that runs past the genome end. The one
// statement of the rule that drm_sw_align_region (capi.cpp) and the kernels (sw_wave.h) both compile; at flank 0 it is
// the window itself.
constexpr int kAlignMaxLen = 256; // longest query and region of the alignment kernels
DRM_HOST_DEVICE inline GenomeRegion align_region(uint64_t w, int64_t glen, int32_t ref_len, int32_t flank)
{
    GenomeRegion r{0, 0, (int32_t)(w & 1u)};
    const uint64_t pos = w >> 1;
    if (pos + (uint64_t)ref_len > (uint64_t)glen)
        return r;
    const int64_t s = (int64_t)pos - flank, e = (int64_t)pos + ref_len + flank;
    r.start = s > 0 ? s : 0;
    r.len = (int32_t)((e < glen ? e : glen) - r.start);
    return r;
}
// The aligners' limits, `what` naming the kernel in the message (null: drm_sw_align_region, which runs none). At
// argument time: a flank is not negative and needs a genome handle (DRM_ERR_ARG), and the region fits the kernels
// (DRM_ERR_UNSUPPORTED) ...
void check_align_flank(const char *what, int32_t ref_len, int32_t flank, bool genome);
// ... and at launch time, when the longest query is known: both sides within kAlignMaxLen (DRM_ERR_UNSUPPORTED)
void check_align_launch(const char *what, int32_t ref_len, int32_t flank, int max_qlen);

// Mate rescue (include/drm_hip.h, drm_mate_rescue): the region of one anchor id, the one statement of the rule that
// the host entry points (read_rules.cpp) and the kernel (mate_rescue.hip) both compile. dlo / dhi are
// max(0, min_tlen - ref_len) and max_tlen - ref_len.
constexpr int kRescueMaxRows = 2048; // longest region: 11 bits of row in the kernel's best-cell key
DRM_HOST_DEVICE inline GenomeRegion rescue_region(uint64_t w, int64_t glen, int32_t ref_len, int64_t dlo, int64_t dhi)
{
    GenomeRegion r{0, 0, (int32_t)(1u - (uint32_t)(w & 1u))};
    const uint64_t a = w >> 1;
    if (dhi < dlo || glen < 0 || a + (uint64_t)ref_len > (uint64_t)glen)
        return r;
    const int64_t pos = (int64_t)a; // <= glen from here on: nothing below overflows
    int64_t s, e;
    if (r.reverse) {
        s = pos + dlo;
        e = pos + dhi + ref_len;
        s = s < glen ? s : glen;
    } else {
        s = pos - dhi;
        e = pos - dlo + ref_len;
        s = s > 0 ? s : 0;
    }
    e = e < glen ? e : glen;
    if (e <= s)
        return r;
    r.start = s;
    r.len = (int32_t)(e - s);
    return r;
}
// drm_pair_hits' ranges of ref_len and the template lengths (DRM_ERR_ARG) ...
void check_pair_params(const drm_pair_params *p);
// ... and the rescue's row cap beside them; returns dlo / dhi
void check_rescue_params(const drm_pair_params *p, int64_t &dlo, int64_t &dhi);
// drm_sw_scoring's accepted ranges (drm_sw_align_affine, drm_mate_rescue; DRM_ERR_ARG)
void check_scoring(const drm_sw_scoring *sc);

// Mapping quality (include/drm_hip.h, drm_mapq_value): the one statement of the formula that the host entry points
// (read_rules.cpp) and the kernels (mapq.hip) both compile. Arguments within [-2^20, 2^20]: 60 * 2^20 * 2^20 < 2^63.
DRM_HOST_DEVICE inline int32_t mapq_value(int64_t s1, int64_t sub, int64_t n_sub, int64_t full, int64_t min_score)
{
    if (s1 <= 0 || full <= 0)
        return 0;
    const int64_t c = s1 < full ? s1 : full, s2 = sub > min_score ? sub : min_score;
    if (c <= s2)
        return 0;
    int64_t q = (60 * (c - s2) * c) / ((c - min_score) * full);
    for (int64_t x = n_sub + 1; x > 1; x >>= 1) // 3 * floor(log2(n_sub + 1))
        q -= 3;
    return (int32_t)(q < 0 ? 0 : q > 60 ? 60 : q);
}
// drm_mapq_params' accepted ranges (DRM_ERR_ARG)
void check_mapq_params(const drm_mapq_params *p);

// Duplicate set (include/drm_hip.h, drm_dupset): the slot hash of a key (lo, hi), the one statement that the kernels
// (dup_set.hip) and drm_dup_slot compile: splitmix64's finaliser over lo ^ rotl(hi, 32); the slot is its low bits.
DRM_HOST_DEVICE inline uint64_t dup_hash(uint64_t lo, uint64_t hi)
{
    uint64_t z = lo ^ ((hi << 32) | (hi >> 32));
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

void build_hnswpq(const float *x, int64_t n, int d, int M_pq, int nbits, int M_hnsw, int efc, double sample_rate,
                  int nthreads, uint64_t seed, const std::string &path);
// Shared by the CPU builder (builder.cpp) and the GPU builder (builder_gpu.hip):
// create_training_set's evenly spaced rows (src/hnswpq/index.cpp:57-84), subsampled to 256 * ksub;
std::vector<size_t> pq_training_rows(int64_t n, double sample_rate, int ksub, uint64_t seed);
// k-means (25 iterations) per sub-quantizer on rows [n_fit][d] -> centroids [M][2^nbits][d / M];
void pq_train_subspaces(const float *rows, size_t n_fit, int d, int M, int nbits, uint64_t seed, int nthreads,
                        float *centroids);
// HNSW::set_default_probas + random_level for n nodes: fills assign_probas, cum_nneighbor_per_level,
// levels (level + 1) and offsets of ix; returns the top level.
int hnsw_assign_levels(HnswPqHost &ix, int64_t n, int M_hnsw, uint64_t seed);
// GPU construction (builder_gpu.hip) from device-resident vectors d_x [n][d]: same file layout and
// levels as build_hnswpq, PQ trained on the host, codes and graph built on `device`.
void build_hnswpq_gpu(const float *d_x, int64_t n, int d, int M_pq, int nbits, int M_hnsw, int efc,
                      double sample_rate, uint64_t seed, int device, const std::string &path);
void embed_kmer3(const uint8_t *seqs, const int64_t *off, const int32_t *len, int64_t n, int dim, uint64_t seed,
                 float *out);
// the [64 x dim] N(0,1) projection of the stand-in embedder (splitmix64(seed) + Box-Muller)
std::vector<double> kmer3_matrix(int dim, uint64_t seed);
constexpr uint64_t kEmbedSeed = 42; // seed of the stand-in embedder used by the CLIs

// ---------------------------------------------------------------------------------------------
// Read encoder (encoder.cpp): the reference's OpenVINO GRU model (models/finetuned_sgn33-new-a-Apr6.xml,
// src/inference/fast_model.cpp), f16 tensors as the IR stores them.
// ---------------------------------------------------------------------------------------------
constexpr int kTokenHashes = 96; // hashToken range backed by _Tok2Index (includes/inference/preprocess.hpp:32-49)

struct EncoderHost {
    int32_t hidden = 64, emb_dim = 64, max_len = 123; // config.hpp:21 (MAX_LEN), the IR's GRU/embedding sizes
    float h0 = 0.f;
    std::vector<uint16_t> vocab_rows; // [1 + 96] vocabulary id of each embedding row (token_vocab_rows)
    std::vector<uint16_t> emb_rows;   // [rows][emb_dim] f16 bits
    std::vector<uint16_t> W[2], R[2], B[2]; // f16 bits: W [2][3H][in], R [2][3H][H], B [2][4H] (zrh)
    int in_dim(int layer) const { return layer == 0 ? emb_dim : 2 * hidden; }
};
std::vector<uint16_t> token_vocab_rows();
EncoderHost read_encoder(const std::string &path); // .xml (IR + sibling .bin) or .drmenc; throws Error
// Model the CLIs embed sequences with: DRM_ENCODER=<.xml|.drmenc> ("kmer3" or empty: the 3-mer stand-in),
// else the reference's Config::Inference::MODEL_PATH relative to the working directory when it exists
// (includes/utils/config.hpp:18), else "" (stand-in).
std::string encoder_model_path();
// Vectorizer::vectorize on `device` for host sequences: out [n][128]
void vectorize_host(const std::string &model, int device, const std::vector<std::string> &seqs, float *out);
void write_encoder(const EncoderHost &e, const std::string &path);

} // namespace drm
