// tests/sam_writer_driver.cpp -- the SAM writers (drm::write_sam_block / drm::write_sam_pairs) on inputs built in
// code, one file per named case: `sam_writer_driver <dir>` writes <dir>/<case>.sam, which
// tests/test_sam_writer_cpu.py compares byte for byte with tests/golden/sam_writer/. Host only, no GPU: the records,
// operation words and MD words are written down here, not computed, and only what the writers check about them holds.
// `sam_writer_driver --time <file>` writes one large block of reads and one of pairs and prints milliseconds.
#include <chrono>
#include <cstdio>
#include <fstream>
#include <functional>

#include "drm_internal.h"

static std::string g_last_error;
void drm::set_last_error(const std::string &msg) { g_last_error = msg; }

namespace {

// ------------------------------------------------------------------------------------------ inputs
constexpr uint32_t M(uint32_t n) { return n << 4; }            // operation words
constexpr uint32_t I(uint32_t n) { return (n << 4) | 1u; }
constexpr uint32_t D(uint32_t n) { return (n << 4) | 2u; }
constexpr uint32_t N(uint32_t n) { return n << 4; }            // MD words: a number, a mismatch, a deleted base
constexpr uint32_t X(char c) { return ((uint32_t)c << 4) | 1u; }
constexpr uint32_t DEL(char c) { return ((uint32_t)c << 4) | 2u; }

// one row of a block: its window id, record, operations, region, MD words, contig and MAPQ
struct Row {
    uint64_t id = 0;
    drm_sw_alignment a{0, 0, 0, 0, 0, 0, 0, 1};
    std::vector<uint32_t> ops;
    int64_t region_start = 0;
    int32_t region_len = 0;
    std::vector<uint32_t> md;
    int32_t contig = 0, mapq = 0;
};
// a row that holds an alignment: q_begin / q_end count in the tagged query
Row row(uint64_t id, int32_t score, int32_t ref_begin, int32_t ref_end, int32_t q_begin, int32_t q_end, int32_t nm,
        std::vector<uint32_t> ops, int32_t mapq = 0)
{
    Row r;
    r.id = id;
    r.a = drm_sw_alignment{score, ref_begin, ref_end, q_begin, q_end, nm, (int32_t)ops.size(), 0};
    r.ops = std::move(ops);
    r.mapq = mapq;
    return r;
}
Row no_alignment(uint64_t id, int32_t mapq = 0) // a status-1 record
{
    Row r;
    r.id = id;
    r.mapq = mapq;
    return r;
}
Row in_region(Row r, int64_t start, int32_t len)
{
    r.region_start = start;
    r.region_len = len;
    return r;
}
Row with_md(Row r, std::vector<uint32_t> words)
{
    r.md = std::move(words);
    return r;
}
Row on_contig(Row r, int32_t c)
{
    r.contig = c;
    return r;
}

// the rows of a block as the arrays the writers read
struct Flat {
    std::vector<uint64_t> ids;
    std::vector<drm_sw_alignment> rec;
    std::vector<uint32_t> ops, md_words;
    std::vector<int64_t> ops_off, region_start, md_off;
    std::vector<int32_t> region_len, contig, mapq;
    std::vector<drm_sw_md> md;
    explicit Flat(const std::vector<Row> &rows)
    {
        for (const Row &r : rows) {
            ids.push_back(r.id);
            rec.push_back(r.a);
            ops_off.push_back((int64_t)ops.size());
            ops.insert(ops.end(), r.ops.begin(), r.ops.end());
            region_start.push_back(r.region_start);
            region_len.push_back(r.region_len);
            md_off.push_back((int64_t)md_words.size());
            md_words.insert(md_words.end(), r.md.begin(), r.md.end());
            md.push_back(drm_sw_md{(int32_t)r.md.size(), 0, 0, 0, 0, r.a.status == 1 ? 1 : r.md.empty() ? 3 : 0});
            contig.push_back(r.contig);
            mapq.push_back(r.mapq);
        }
        ops.push_back(0); // never empty: data() stays a valid pointer
        md_words.push_back(0);
    }
};

struct Reads {
    std::vector<std::string> seqs, ids, quals;
};
// which of a block's optional inputs the call passes
struct Mode {
    bool aln = false, region = false, md = false, contigs = false, mapq = false, quals = false, loci = false,
         xa = false;
};
struct ReadBlock {
    size_t q0, nq, k;
    std::vector<int32_t> counts; // [nq]
    std::vector<Row> rows;       // [nq * k]
    std::vector<uint8_t> dup;    // [nq], DRM_SAM_DUP; empty = the call passes none
};
struct PairBlock {
    size_t q0, npairs;
    std::vector<int32_t> counts, proper; // [2 * npairs], [npairs]
    std::vector<Row> rows;               // [2 * npairs]
    size_t xa_width = 0;                 // Mode::xa: the alternates of every row, from slot 0
    std::vector<int32_t> xa_counts;      // [2 * npairs]
    std::vector<Row> xa_rows;            // [2 * npairs * xa_width]
    std::vector<uint8_t> dup;            // [2 * npairs], DRM_SAM_DUP; empty = the call passes none
};

const std::vector<drm::FastaContig> kContigs = {{"chrA", 0, 400}, {"chrB", 405, 600}};
constexpr size_t kRefLen = 12;

drm::SamAlignments view(const Flat &f, const Mode &m)
{
    drm::SamAlignments v{f.rec.data(), f.ops.data(), f.ops_off.data()};
    if (m.region) {
        v.region_start = f.region_start.data();
        v.region_len = f.region_len.data();
    }
    if (m.md) {
        v.md = f.md.data();
        v.md_words = f.md_words.data();
        v.md_off = f.md_off.data();
    }
    return v;
}

// ------------------------------------------------------------------------------------------ the two calls
// what both calls say about a block
drm::SamBlock block(const std::string &path, bool header, const Reads &r, size_t q0, const Flat &f, const Mode &m,
                    size_t ref_len, const drm::SamAlignments *av, const drm::SamContigs *sc,
                    const std::vector<uint8_t> &dup)
{
    drm::SamBlock b;
    b.path = path;
    b.header = header;
    b.ref_len = ref_len;
    b.queries = &r.seqs;
    b.query_ids = &r.ids;
    b.quals = m.quals ? &r.quals : nullptr;
    b.q0 = q0;
    b.ids = f.ids.data();
    b.aln = m.aln ? av : nullptr;
    b.mapq = m.mapq ? f.mapq.data() : nullptr;
    b.ctg = m.contigs ? sc : nullptr;
    b.dup = dup.empty() ? nullptr : dup.data();
    return b;
}

void write_reads(const std::string &path, bool header, const Reads &r, const ReadBlock &b, const Mode &m,
                 size_t ref_len = kRefLen)
{
    const Flat f(b.rows);
    const drm::SamAlignments av = view(f, m);
    const drm::SamContigs sc{&kContigs, f.contig.data()};
    drm::write_sam_block(block(path, header, r, b.q0, f, m, ref_len, &av, &sc, b.dup), b.nq, b.counts.data(), b.k,
                         m.loci, m.xa);
}

void write_pairs(const std::string &path, bool header, const Reads &r, const PairBlock &b, const Mode &m,
                 size_t ref_len = kRefLen)
{
    const Flat f(b.rows), xf(b.xa_rows);
    const drm::SamAlignments av = view(f, m), xav = view(xf, m);
    const drm::SamContigs sc{&kContigs, f.contig.data()}, xsc{&kContigs, xf.contig.data()};
    const drm::SamXa xa{xf.ids.data(), b.xa_counts.data(), b.xa_width, 0, &xav, m.contigs ? &xsc : nullptr};
    drm::write_sam_pairs(block(path, header, r, b.q0, f, m, ref_len, &av, &sc, b.dup), b.npairs,
                         b.counts.data(), b.proper.data(), m.xa ? &xa : nullptr);
}

// ------------------------------------------------------------------------------------------ single reads
// six reads of ten bases or fewer; read 2 has an empty id, read 3 is untagged, read 4 has an empty quality line and
// read 5 has no id at all (the id list is one short)
Reads six_reads()
{
    return {{"<ACGTACGTAC>", "<GGGTTTAAAC>", "<TTTTACGT>", "ACGTTGCA", "<CCCCAGAGTT>", "<AGTCCGATTA>"},
            {"r0", "r1", "", "r3", "r4"},
            {"ABCDEFGHIJ", "abcdefghij", "01234567", "KLMNOPQR", "", "xyzXYZxyzX"}};
}

void case_pseudo(const std::string &path, bool mapq)
{
    const Reads r = six_reads();
    Mode m;
    m.quals = true;
    m.mapq = mapq;
    // k = 2, counts 2, 0, 1: forward and reverse ids, unused slots behind the count
    write_reads(path, true, r, {0, 3, 2, {2, 0, 1},
                                {no_alignment(20, 37), no_alignment(43, 3), no_alignment(7, 60), no_alignment(999, 1),
                                 no_alignment(997, 2), no_alignment(998, 4)}}, m);
    write_reads(path, false, r, {3, 3, 2, {1, 2, 1},
                                 {no_alignment(0, 11), no_alignment(5, 12), no_alignment(101, 0), no_alignment(100, 13),
                                  no_alignment(1ull << 33, 59), no_alignment(3, 14)}}, m);
}

// window mode, k = 2. Tagged queries of 12 bytes: q_begin 1 and q_end 11 leave no clip.
std::vector<ReadBlock> aligned_blocks()
{
    return {{0, 3, 2, {2, 1, 1},
             {// read 0: forward with clips 2 and 2, then a reverse secondary with a trailing clip only
              with_md(row(200, 4, 1, 8, 3, 9, 3, {M(3), I(1), M(2), D(2)}, 40), {N(3), X('A'), N(1), DEL('C'), DEL('G'), N(0)}),
              with_md(row(101, 6, 2, 10, 1, 8, 1, {M(4), D(1), M(3)}, 17), {N(4), DEL('T'), N(3)}),
              // read 1: reverse with clips 1 and 3: the operations turn round and the clips swap
              with_md(row(61, 5, 0, 5, 2, 8, 1, {M(2), I(1), M(3)}, 23), {N(1), X('G'), N(3)}), no_alignment(0),
              // read 2: a reverse hit without an alignment
              no_alignment(11, 33), no_alignment(0)}},
            {3, 3, 2, {1, 1, 0},
             {// read 3: untagged, the whole query aligned
              with_md(row(14, 8, 3, 11, 0, 8, 0, {M(8)}, 60), {N(8)}), no_alignment(0),
              // read 4: reverse, an empty quality line
              with_md(row(2001, 7, 0, 12, 1, 11, 2, {M(5), I(2), D(4), M(3)}, 9),
                      {N(2), X('C'), N(2), DEL('A'), DEL('A'), DEL('C'), DEL('T'), X('N'), N(2)}),
              no_alignment(0),
              // read 5: no rows
              no_alignment(0), no_alignment(0)}}};
}

// the same rows over flanked regions; row 0's region starts where its window does not
std::vector<ReadBlock> region_blocks()
{
    std::vector<ReadBlock> b = aligned_blocks();
    const int64_t start[2][6] = {{90, 40, 27, 0, 0, 0}, {7, 0, 990, 0, 0, 0}};
    const int32_t len[2][6] = {{20, 22, 18, 0, 0, 0}, {12, 0, 32, 0, 0, 0}};
    for (size_t x = 0; x < 2; ++x)
        for (size_t i = 0; i < 6; ++i)
            b[x].rows[i] = in_region(b[x].rows[i], start[x][i], len[x][i]);
    return b;
}

void case_reads(const std::string &path, std::vector<ReadBlock> blocks, const Mode &m)
{
    const Reads r = six_reads();
    for (size_t x = 0; x < blocks.size(); ++x)
        write_reads(path, x == 0, r, blocks[x], m);
}

// two contigs: rows on either, POS local to the contig; read 2 loses its row
std::vector<ReadBlock> contig_blocks(std::vector<ReadBlock> b)
{
    const int32_t c[2][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, 1, 0, 0, 0}};
    for (size_t x = 0; x < 2; ++x)
        for (size_t i = 0; i < 6; ++i)
            b[x].rows[i] = on_contig(b[x].rows[i], c[x][i]);
    b[0].rows[0].id = 2 * 410; // read 0's primary on chrB, its secondary stays on chrA
    b[0].rows[0].region_start += 405;
    b[0].rows[0].contig = 1;
    b[0].counts[2] = 0;
    return b;
}

// lines per locus, k = 3 loci: read 0 has a status-1 alternate and a good one, read 1 only status-1 alternates,
// read 2 no locus, read 3 one locus, read 4 a status-1 primary in front of a good alternate, read 5 two good alternates
std::vector<ReadBlock> loci_blocks()
{
    const Row fwd = in_region(with_md(row(200, 9, 1, 9, 2, 10, 1, {M(8)}, 40), {N(3), X('T'), N(4)}), 95, 20);
    const Row rev = in_region(with_md(row(521, 6, 2, 10, 1, 8, 1, {M(4), D(1), M(3)}, 0), {N(4), DEL('T'), N(3)}), 250, 22);
    const Row far = on_contig(in_region(with_md(row(1500, 5, 0, 5, 2, 8, 2, {M(2), I(1), M(3)}, 0), {N(1), X('G'), N(3)}),
                                         740, 18), 1);
    return {{0, 3, 3, {3, 2, 0},
             {fwd, no_alignment(30), far, rev, no_alignment(77), no_alignment(0), no_alignment(0), no_alignment(0),
              no_alignment(0)}},
            {3, 3, 3, {1, 2, 3},
             {in_region(with_md(row(14, 8, 3, 11, 0, 8, 0, {M(8)}, 60), {N(8)}), 5, 14), no_alignment(0), no_alignment(0),
              no_alignment(41, 5), rev, no_alignment(0), far, fwd, rev}}};
}

// DRM_SAM_DUP on reads 0, 2 and 4 (tests/test_sam_writer_cpu.py, DUP_READS): a read with a status-1 secondary and a
// good one, a read without a locus, and a read whose primary holds no alignment
std::vector<ReadBlock> loci_dup_blocks()
{
    std::vector<ReadBlock> b = loci_blocks();
    b[0].dup = {1, 0, 1};
    b[1].dup = {0, 1, 0};
    return b;
}

// ------------------------------------------------------------------------------------------ pairs
// six pairs; the reads of pair 5 have no id
Reads pair_reads()
{
    Reads r;
    const char *s[4] = {"<ACGTACGTAC>", "<GGGTTTAAAC>", "<TTTTACGTCA>", "CCCCAGAGTT"};
    for (int i = 0; i < 12; ++i) {
        r.seqs.push_back(s[i % 4]);
        r.ids.push_back(i < 10 ? "p" + std::to_string(i / 2) : "");
        r.quals.push_back(i == 3 ? std::string() : std::string("ABCDEFGHIJ").substr(0, 10 - (size_t)(i % 2)) + "!");
        r.quals.back().resize(10, '#');
    }
    return r;
}

std::vector<PairBlock> pair_blocks()
{
    const Row f100 = with_md(row(200, 9, 0, 10, 1, 11, 1, {M(10)}, 50), {N(4), X('A'), N(5)});
    const Row r150 = with_md(row(301, 7, 1, 10, 2, 11, 1, {M(4), I(1), D(1), M(4)}, 48), {N(4), DEL('G'), N(4)});
    const Row f160 = with_md(row(320, 6, 2, 9, 3, 10, 0, {M(7)}, 12), {N(7)});
    const Row untagged = with_md(row(642, 10, 1, 11, 0, 10, 0, {M(10)}, 31), {N(10)});
    PairBlock a{0, 3, {1, 1, 1, 1, 1, 0}, {1, 0, 0},
                {f100, r150,                  // pair 0: a proper FR pair
                 f160, untagged,              // pair 1: both forward, not proper
                 r150, no_alignment(0, 7)}};  // pair 2: mate 2 without a hit takes mate 1's RNAME and POS
    PairBlock b{6, 3, {0, 0, 1, 1, 1, 1}, {0, 1, 1},
                {no_alignment(0, 5), no_alignment(0, 6), // pair 3: neither mate has a hit
                 no_alignment(41, 9), f160,              // pair 4: a counted row with a status-1 record
                 r150, untagged}};                       // pair 5: proper, the reverse mate first, no read ids
    return {a, b};
}

// DRM_SAM_DUP on pairs 0, 2 and 5 (DUP_PAIRS), the pair's answer on both of its rows: a proper pair, a pair with one
// mate unmapped, and the pair without read ids
std::vector<PairBlock> pair_dup_blocks()
{
    std::vector<PairBlock> b = pair_blocks();
    b[0].dup = {1, 1, 0, 0, 1, 1};
    b[1].dup = {0, 0, 0, 0, 1, 1};
    return b;
}

// mates on two contigs (pair 0, called proper), on one contig (pairs 1 and 5), one mate unmapped beside chrB (pair 4)
std::vector<PairBlock> pair_contig_blocks(std::vector<PairBlock> b)
{
    b[0].rows[1] = on_contig(b[0].rows[1], 1);
    b[0].rows[1].id = 2 * 600 + 1;
    b[1].rows[3] = on_contig(b[1].rows[3], 1);
    b[1].rows[3].id = 2 * 420;
    b[1].rows[4] = on_contig(b[1].rows[4], 1);
    b[1].rows[4].id = 2 * 800 + 1;
    b[1].rows[5] = on_contig(b[1].rows[5], 1);
    b[1].rows[5].id = 2 * 830;
    return b;
}

// every row over a flanked region, and two slots of alternates per row: slot 0 repeats the row's own locus
std::vector<PairBlock> pair_xa_blocks(std::vector<PairBlock> b)
{
    for (PairBlock &blk : b) {
        blk.xa_width = 2;
        for (size_t r = 0; r < blk.rows.size(); ++r) {
            Row &own = blk.rows[r];
            own = in_region(own, (int64_t)(own.id / 2) - 3, 18);
            Row other = own;
            other.id ^= 1u;
            other.region_start = own.contig ? 410 : 33;
            other.contig = own.contig;
            other.a.nm += 2;
            const bool mapped = blk.counts[r] > 0 && own.a.status == 0;
            blk.xa_counts.push_back(!mapped ? 0 : r % 3 == 0 ? 1 : 2);
            blk.xa_rows.push_back(own);
            blk.xa_rows.push_back(r % 3 == 1 ? no_alignment(own.id) : other);
        }
    }
    return b;
}

void case_pairs(const std::string &path, const std::vector<PairBlock> &blocks, const Mode &m)
{
    const Reads r = pair_reads();
    for (size_t x = 0; x < blocks.size(); ++x)
        write_pairs(path, x == 0, r, blocks[x], m);
}

// ------------------------------------------------------------------------------------------ large blocks
// n copies of one aligned read of 150 bases, region, MD, contigs and quality lines on
void big_reads(size_t n, Reads &r, ReadBlock &b)
{
    const std::string read(150, 'C');
    const Row one = on_contig(in_region(with_md(row(2 * 50000 + 1, 133, 3, 153, 2, 150, 5, {M(70), I(1), M(40), D(3), M(37)}, 42),
                                                {N(30), X('A'), N(59), X('T'), N(19), DEL('A'), DEL('C'), DEL('G'), N(37)}),
                                        49990, 170), 1);
    r.seqs.assign(n, "<" + read + ">");
    r.ids.assign(n, "read");
    r.quals.assign(n, std::string(150, 'F'));
    b = ReadBlock{0, n, 1, std::vector<int32_t>(n, 1), std::vector<Row>(n, one)};
}

void big_pairs(size_t npairs, Reads &r, PairBlock &b)
{
    ReadBlock rb;
    big_reads(2 * npairs, r, rb);
    b = PairBlock{0, npairs, rb.counts, std::vector<int32_t>(npairs, 1), rb.rows};
    for (size_t i = 0; i < b.rows.size(); i += 2) { // mate 1 forward and 200 bases to the left
        b.rows[i].id = 2 * 49800;
        b.rows[i].region_start -= 200;
    }
    b.xa_width = 4;
    b.xa_counts.assign(2 * npairs, 3);
    for (size_t i = 0; i < 2 * npairs; ++i)
        for (size_t j = 0; j < 4; ++j)
            b.xa_rows.push_back(j == 1 ? no_alignment(9) : b.rows[i]);
}

void case_flush(const std::string &path) // one call whose text passes the 4 MiB flush four times
{
    Reads r;
    ReadBlock b;
    big_reads(40000, r, b);
    Mode m;
    m.aln = m.region = m.md = m.contigs = m.quals = m.mapq = true;
    write_reads(path, true, r, b, m);
}

// ------------------------------------------------------------------------------------------ errors
void case_errors(const std::string &path, const std::string &scratch)
{
    std::ofstream out(path);
    auto attempt = [&](const char *what, const std::function<void()> &f) {
        try {
            f();
            out << what << ": no error\n";
        } catch (const drm::Error &e) {
            out << what << ": " << e.code << " " << e.what() << "\n";
        }
    };
    const Reads r = six_reads();
    const ReadBlock b = aligned_blocks()[0];
    Mode ctg_only, xa_only, aln;
    ctg_only.contigs = true;
    xa_only.aln = xa_only.xa = true;
    aln.aln = true;
    attempt("contigs without alignments", [&] { write_reads(scratch, true, r, b, ctg_only); });
    attempt("xa without loci", [&] { write_reads(scratch, true, r, b, xa_only); });
    ReadBlock tags = b;
    tags.rows[0].a.q_begin = 0; // the '<' of the tagged query
    attempt("alignment inside the tags", [&] { write_reads(scratch, true, r, tags, aln); });
    attempt("unopenable path", [&] { write_reads("/no-such-directory/of/sam_writer_driver/x.sam", true, r, b, aln); });
    attempt("unopenable path, pairs",
            [&] { write_pairs("/no-such-directory/of/sam_writer_driver/x.sam", false, pair_reads(), pair_blocks()[0], aln); });
}

int time_mode(const std::string &path)
{
    using clock = std::chrono::steady_clock;
    auto ms = [](clock::time_point a, clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    Mode m;
    m.aln = m.region = m.md = m.contigs = m.quals = m.mapq = true;
    Reads r, pr;
    ReadBlock b;
    PairBlock pb;
    big_reads(100000, r, b);
    big_pairs(50000, pr, pb);
    const Flat warm(b.rows); // touch the inputs once
    const auto t0 = clock::now();
    write_reads(path, true, r, b, m);
    const auto t1 = clock::now();
    m.xa = true;
    write_pairs(path, true, pr, pb, m);
    const auto t2 = clock::now();
    std::printf("reads_ms %.2f pairs_ms %.2f total_ms %.2f\n", ms(t0, t1), ms(t1, t2), ms(t0, t2));
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc == 3 && std::string(argv[1]) == "--time")
        return time_mode(argv[2]);
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <output directory> | --time <file>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    auto at = [&](const char *name) { return dir + "/" + name + ".sam"; };
    try {
        Mode m;
        case_pseudo(at("pseudo"), false);
        case_pseudo(at("pseudo_mapq"), true);
        m.aln = m.quals = m.mapq = true;
        case_reads(at("aligned"), aligned_blocks(), m);
        m.mapq = false;
        m.region = true;
        case_reads(at("region"), region_blocks(), m);
        m.region = false;
        m.md = true;
        case_reads(at("md"), aligned_blocks(), m);
        m.md = false;
        m.contigs = m.mapq = true;
        case_reads(at("contigs"), contig_blocks(aligned_blocks()), m);
        m = Mode();
        m.aln = m.loci = m.quals = true;
        case_reads(at("loci_plain"), loci_blocks(), m);
        m.xa = true;
        case_reads(at("loci_xa_plain"), loci_blocks(), m);
        m.region = m.contigs = m.md = m.mapq = true;
        case_reads(at("loci_xa"), loci_blocks(), m);
        m.xa = false;
        case_reads(at("loci"), loci_blocks(), m);
        case_reads(at("loci_dup"), loci_dup_blocks(), m);
        m = Mode();
        m.aln = m.quals = true;
        case_pairs(at("pairs"), pair_blocks(), m);
        case_pairs(at("pairs_dup"), pair_dup_blocks(), m);
        m.mapq = m.md = true;
        case_pairs(at("pairs_mapq"), pair_blocks(), m);
        m.md = false;
        m.contigs = true;
        case_pairs(at("pairs_contigs"), pair_contig_blocks(pair_blocks()), m);
        m.xa = m.region = true;
        case_pairs(at("pairs_xa"), pair_xa_blocks(pair_contig_blocks(pair_blocks())), m);
        m.contigs = false;
        case_pairs(at("pairs_xa_plain"), pair_xa_blocks(pair_blocks()), m);
        case_flush(at("flush"));
        case_errors(at("errors"), at("errors_scratch"));
    } catch (const std::exception &e) {
        std::fprintf(stderr, "sam_writer_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
