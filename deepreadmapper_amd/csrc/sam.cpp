// deepreadmapper_amd/csrc/sam.cpp -- the SAM text: CIGAR / POS and MD of one GPU alignment record, the fields that
// relate the two lines of a pair, and the writers of one block of reads or pairs (drm_internal.h, SamBlock).
// Every line goes through SamLine / append_line, every row's POS and CIGAR through place_row.
// DRM_SAM_SORT=coordinate: SamOut appends the lines to a SamSpool with their sort keys (drm_sam_sort_key) instead of
// writing them, and write_sam_sorted writes the spool in a given order under @HD SO:coordinate. The spool holds the whole
// run in host memory; an external merge for runs that do not fit is not implemented.
// DRM_SAM_FORMAT=bam: SamOut sends every line through SamBlock::bam (drm_internal.h, BamSink; bam.cpp has the encoder
// and the file), to the sink or to the spool, and write_bam_sorted is write_sam_sorted's twin over encoded records.
#include <array>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string_view>
#include <unordered_map>

#include "drm_internal.h"

using namespace drm;

// ------------------------------------------------------------------------------ sequences
static const std::array<char, 128> &comp_table()
{
    static const std::array<char, 128> t = [] {
        std::array<char, 128> x{};
        x['A'] = 'T';
        x['T'] = 'A';
        x['C'] = 'G';
        x['G'] = 'C';
        x['N'] = 'N';
        return x;
    }();
    return t;
}

static void append_reverse_complement(std::string &out, std::string_view seq)
{
    const auto &t = comp_table();
    for (auto it = seq.rbegin(); it != seq.rend(); ++it) {
        unsigned char c = (unsigned char)*it;
        out.push_back(c < 128 ? t[c] : '\0');
    }
}

std::string drm::reverse_complement(const std::string &seq)
{
    std::string rc;
    rc.reserve(seq.size());
    append_reverse_complement(rc, seq);
    return rc;
}

// ----------------------------------------------------------------------- one GPU alignment record
// CIGAR + POS of one drm_sw_alignment record over the region genome[region_start ..+ region_len), reverse-complemented
// when rev (include/drm_hip.h: drm_sam_cigar_region; drm_sam_cigar is the region of a window id)
static void sam_cigar(const drm_sw_alignment &a, const uint32_t *ops, int32_t q_len, int32_t tag_prefix,
                      int32_t tag_postfix, int64_t region_start, int32_t region_len, bool rev, int64_t &pos1,
                      std::string &cigar)
{
    if (a.status != 0)
        throw Error(DRM_ERR_ARG, a.status == 1 ? "the record holds no alignment (status 1)"
                                               : "the record's operations are truncated (status 2): align the pair again "
                                                 "with a larger ops_stride");
    if (a.n_ops < 0 || (a.n_ops > 0 && !ops))
        throw Error(DRM_ERR_ARG, "null operations");
    const int32_t lead = a.q_begin - tag_prefix, trail = (q_len - tag_postfix) - a.q_end;
    if (tag_prefix < 0 || tag_postfix < 0 || lead < 0 || trail < 0)
        throw Error(DRM_ERR_ARG, "the alignment reaches into the query's tags");
    static const char kOp[] = "MID";
    cigar.clear();
    auto clip = [&](int32_t n) {
        if (n > 0)
            cigar += std::to_string(n) + "S";
    };
    clip(rev ? trail : lead);
    for (int32_t x = 0; x < a.n_ops; ++x) {
        const uint32_t w = ops[rev ? a.n_ops - 1 - x : x];
        if ((w & 15u) > 2u)
            throw Error(DRM_ERR_ARG, "operation word " + std::to_string(x) + " is not M, I or D");
        cigar += std::to_string(w >> 4);
        cigar += kOp[w & 15u];
    }
    clip(rev ? lead : trail);
    pos1 = region_start + (rev ? region_len - a.ref_end : a.ref_begin) + 1;
}

extern "C" int drm_sam_cigar_region(const drm_sw_alignment *a, const uint32_t *ops, int32_t q_len, int32_t tag_prefix,
                                    int32_t tag_postfix, int64_t region_start, int32_t region_len, int32_t reverse,
                                    int64_t *pos1, char *cigar, int32_t cigar_cap)
{
    return drm::guarded([&] {
        if (!a || !pos1 || !cigar)
            throw Error(DRM_ERR_ARG, "null argument");
        std::string c;
        int64_t p = 0;
        sam_cigar(*a, ops, q_len, tag_prefix, tag_postfix, region_start, region_len, reverse != 0, p, c);
        if ((int64_t)c.size() + 1 > (int64_t)cigar_cap)
            throw Error(DRM_ERR_ARG, "cigar_cap " + std::to_string(cigar_cap) + " is too small for " +
                                         std::to_string(c.size() + 1) + " bytes");
        std::memcpy(cigar, c.c_str(), c.size() + 1);
        *pos1 = p;
    });
}

extern "C" int drm_sam_cigar(const drm_sw_alignment *a, const uint32_t *ops, int32_t q_len, int32_t tag_prefix,
                             int32_t tag_postfix, int32_t ref_len, uint64_t window_id, int64_t *pos1, char *cigar,
                             int32_t cigar_cap)
{
    return drm_sam_cigar_region(a, ops, q_len, tag_prefix, tag_postfix, (int64_t)(window_id / 2), ref_len,
                                (int32_t)(window_id & 1u), pos1, cigar, cigar_cap);
}

// the MD string of one drm_sw_md record and its words (include/drm_hip.h: drm_sam_md)
static void sam_md(const drm_sw_md &h, const uint32_t *words, bool rev, std::string &md)
{
    if (h.status != 0)
        throw Error(DRM_ERR_ARG, h.status == 2 ? "the record's MD words are truncated (status 2): compute the pair again "
                                                 "with a larger md_stride"
                                               : "the record holds no MD words (status " + std::to_string(h.status) + ")");
    if (h.n_words < 1 || !words)
        throw Error(DRM_ERR_ARG, "an MD stream holds at least one number");
    const auto &comp = comp_table();
    md.clear();
    uint32_t prev = 1; // the kind in front of word x; anything but a number in front of the first
    for (int32_t x = 0; x < h.n_words; ++x) {
        const uint32_t w = words[rev ? h.n_words - 1 - x : x], kind = w & 15u, value = w >> 4;
        if (kind > 2u)
            throw Error(DRM_ERR_ARG, "MD word " + std::to_string(x) + " is not a number, a mismatch or a deleted base");
        if (kind == 0u) {
            if (prev == 0u)
                throw Error(DRM_ERR_ARG, "MD words " + std::to_string(x - 1) + " and " + std::to_string(x) +
                                             " are both numbers");
            md += std::to_string(value);
        } else {
            if (x == 0 || x == h.n_words - 1)
                throw Error(DRM_ERR_ARG, "an MD stream starts and ends with a number");
            const uint32_t base = !rev ? value : value < 128u ? (uint32_t)(unsigned char)comp[value] : 0u;
            if (base < 'A' || base > 'Z')
                throw Error(DRM_ERR_ARG, "MD word " + std::to_string(x) + " holds no base letter");
            if (kind == 2u && prev != 2u)
                md += '^';
            md += (char)base;
        }
        prev = kind;
    }
}

extern "C" int drm_sam_md(const drm_sw_md *h, const uint32_t *words, int32_t reverse, char *md, int32_t md_cap)
{
    return drm::guarded([&] {
        if (!h || !md)
            throw Error(DRM_ERR_ARG, "null argument");
        std::string s;
        sam_md(*h, words, reverse != 0, s);
        if ((int64_t)s.size() + 1 > (int64_t)md_cap)
            throw Error(DRM_ERR_ARG, "md_cap " + std::to_string(md_cap) + " is too small for " +
                                         std::to_string(s.size() + 1) + " bytes");
        std::memcpy(md, s.c_str(), s.size() + 1);
    });
}

// ----------------------------------------------------------------------- paired SAM (include/drm_hip.h)
static void sam_pair_fields(const drm_sam_mate in[2], bool proper, drm_sam_mate_fields out[2])
{
    for (int m = 0; m < 2; ++m)
        if (in[m].mapped && (in[m].pos1 < 1 || in[m].ref_span < 1))
            throw Error(DRM_ERR_ARG, "mate " + std::to_string(m + 1) + " is mapped with pos1 " +
                                         std::to_string(in[m].pos1) + ", ref_span " + std::to_string(in[m].ref_span) +
                                         ": both must be >= 1");
    const bool both = in[0].mapped && in[1].mapped, any = in[0].mapped || in[1].mapped;
    int64_t len = 0;
    if (both)
        len = std::max(in[0].pos1 + in[0].ref_span - 1, in[1].pos1 + in[1].ref_span - 1) -
              std::min(in[0].pos1, in[1].pos1) + 1;
    for (int m = 0; m < 2; ++m) {
        const drm_sam_mate &self = in[m], &mate = in[1 - m];
        drm_sam_mate_fields &o = out[m];
        o.flag = 0x1 | (m == 0 ? 0x40 : 0x80) | (self.mapped ? 0 : 0x4) | (mate.mapped ? 0 : 0x8) |
                 (self.mapped && self.reverse ? 0x10 : 0) | (mate.mapped && mate.reverse ? 0x20 : 0) |
                 (proper && both ? 0x2 : 0);
        o.has_rname = any ? 1 : 0;
        o.pos = self.mapped ? self.pos1 : mate.mapped ? mate.pos1 : 0;
        o.pnext = mate.mapped ? mate.pos1 : self.mapped ? self.pos1 : 0;
        const bool left = self.pos1 < mate.pos1 || (self.pos1 == mate.pos1 && m == 0);
        o.tlen = both ? (left ? len : -len) : 0;
    }
}

extern "C" int drm_sam_pair_fields(const drm_sam_mate in[2], int proper, drm_sam_mate_fields out[2])
{
    return drm::guarded([&] {
        if (!in || !out)
            throw Error(DRM_ERR_ARG, "null argument");
        sam_pair_fields(in, proper != 0, out);
    });
}

// ----------------------------------------------------------------------- the writers' shared parts
namespace {

// Where one row puts its read: the read itself (the query without format_fastq's tags; an untagged .txt query is the
// read), its strand, and for a record that holds an alignment the 1-based leftmost position in the contig's own
// coordinates (the genome's without a contig) and the CIGAR.
struct Placed {
    std::string_view read;
    bool mapped = false, reverse = false;
    int64_t pos1 = 0;
    std::string cigar = "*";
    const FastaContig *contig = nullptr;
};

Placed place_row(const SamAlignments *aln, size_t row, uint64_t id, const std::string &tagged, size_t ref_len,
                 const FastaContig *contig)
{
    const int pre = !tagged.empty() && tagged.front() == '<', post = tagged.size() > 1 && tagged.back() == '>';
    Placed p;
    p.read = std::string_view(tagged).substr((size_t)pre, tagged.size() - (size_t)pre - (size_t)post);
    if (!aln) // a read without a row: the read alone
        return p;
    p.reverse = (id & 1u) != 0;
    p.contig = contig;
    const drm_sw_alignment &a = aln->rec[row];
    if (a.status == 1)
        return p;
    // over the row's flanked region (drm_sw_align_affine) when the block has regions, else over the window of the id
    const bool region = aln->region_start != nullptr;
    sam_cigar(a, aln->ops + aln->ops_off[row], (int32_t)tagged.size(), pre, post,
              region ? aln->region_start[row] : (int64_t)(id / 2), region ? aln->region_len[row] : (int32_t)ref_len,
              p.reverse, p.pos1, p.cigar);
    p.pos1 -= contig ? contig->start : 0;
    p.mapped = true;
    return p;
}

const FastaContig *contig_of(const SamContigs *ctg, size_t row)
{
    return ctg ? &(*ctg->table)[(size_t)ctg->row_contig[row]] : nullptr;
}

void append_line(std::string &buf, const SamLine &l)
{
    auto column = [&](std::string_view s) { buf.append(s).push_back('\t'); };
    column(l.qname);
    column(std::to_string(l.flag));
    column(l.rname);
    column(std::to_string(l.pos));
    column(std::to_string(l.mapq));
    column(l.cigar);
    column(l.rnext);
    column(std::to_string(l.pnext));
    column(std::to_string(l.tlen));
    if (l.read.empty())
        buf += '*';
    else if (l.reversed)
        append_reverse_complement(buf, l.read);
    else
        buf += l.read;
    buf += '\t';
    if (l.qual.empty())
        buf += '*';
    else if (l.reversed)
        buf.append(l.qual.rbegin(), l.qual.rend());
    else
        buf += l.qual;
    buf += l.tags;
    buf += '\n';
}

// the tags of a mapped row: AS and NM of its record, MD when the block carries MD records, then `xa`
std::string mapped_tags(const SamAlignments &aln, size_t row, bool rev, const std::string &xa)
{
    std::string t = "\tAS:i:" + std::to_string(aln.rec[row].score) + "\tNM:i:" + std::to_string(aln.rec[row].nm);
    if (aln.md) {
        std::string md;
        sam_md(aln.md[row], aln.md_words + aln.md_off[row], rev, md);
        t.append("\tMD:Z:").append(md);
    }
    t += xa;
    return t;
}

// DRM_SAM_LOCI: "\tXA:Z:" and one "RNAME,<+|->POS,CIGAR,NM;" per alternate of block row `read` that holds an
// alignment; empty when none does (drm_internal.h, SamXa)
std::string xa_tag(const SamXa &xa, size_t read, const std::string &tagged, const SamBlock &b)
{
    std::string tag;
    for (size_t j = xa.first; j < xa.width && (int64_t)j < (int64_t)xa.counts[read]; ++j) {
        const size_t row = read * xa.width + j;
        if (xa.aln->rec[row].status == 1) // such a row may have no contig either
            continue;
        const Placed p = place_row(xa.aln, row, xa.ids[row], tagged, b.ref_len, contig_of(xa.ctg, row));
        tag += tag.empty() ? "\tXA:Z:" : "";
        tag += (p.contig ? p.contig->name : b.ref_name) + "," + (p.reverse ? "-" : "+") + std::to_string(p.pos1) + "," +
               p.cigar + "," + std::to_string(xa.aln->rec[row].nm) + ";";
    }
    return tag;
}

// QNAME of query g: its id, or S1/<number>/0 for a query without one
std::string qname_of(const SamBlock &b, size_t g, size_t number)
{
    return b.query_ids && g < b.query_ids->size() && !(*b.query_ids)[g].empty() ? (*b.query_ids)[g]
                                                                                : "S1/" + std::to_string(number) + "/0";
}

// @HD with the given sort order, then @SQ: the reference's one line, or with a contig table one line per contig in
// file order
void write_header(std::ostream &out, const SamBlock &b, const char *order)
{
    out << "@HD\tVN:1.0\tSO:" << order << "\n";
    if (!b.ctg)
        out << "@SQ\tSN:" << b.ref_name << "\tLN:" << b.ref_len << "\n";
    else
        for (const FastaContig &c : *b.ctg->table)
            out << "@SQ\tSN:" << c.name << "\tLN:" << c.len << "\n";
}

// exactly the text write_header writes: what the BAM header holds
std::string header_text(const SamBlock &b, const char *order)
{
    std::ostringstream text;
    write_header(text, b, order);
    return text.str();
}

uint64_t sam_sort_key(int64_t tid, int64_t pos, bool reverse)
{
    if (tid == -1)
        return ~0ull;
    if (tid < 0 || tid >= ((int64_t)1 << 29))
        throw Error(DRM_ERR_ARG, "tid " + std::to_string(tid) + " outside [-1, 2^29)");
    if (pos < 0 || pos >= ((int64_t)1 << 33))
        throw Error(DRM_ERR_ARG, "pos " + std::to_string(pos) + " outside [0, 2^33)");
    return ((((uint64_t)tid << 33) | (uint64_t)pos) << 1) | (reverse ? 1u : 0u);
}

// The block's file: opened to truncate (with the header) or to append; the text is collected and written out whenever
// it passes 4 MiB at the end of a record, and after the last one. A block that throws leaves the rest unwritten.
// With a spool (DRM_SAM_SORT=coordinate) no file is touched: every line goes to the spool's text, with its offset and
// its sort key (drm_sam_sort_key of the index of its RNAME among the @SQ lines, its POS and its flag's bit 16).
// With a BAM sink (DRM_SAM_FORMAT=bam) a line is its BAM record (BamSink::encode) wherever its text would have gone: in
// the spool, or in the sink, which the block with the header opens and which compresses and writes on its own schedule.
class SamOut {
    std::ofstream out;
    std::string buf;
    SamSpool *spool;
    BamSink *bam;
    SamRefIds tid; // spool or BAM: RNAME -> its first @SQ line
    void put(std::string &to, const SamLine &l)
    {
        if (bam)
            bam->encode(l, tid, to);
        else
            append_line(to, l);
    }
public:
    explicit SamOut(const SamBlock &b) : spool(b.spool), bam(b.bam)
    {
        if (spool || bam) {
            if (!b.ctg)
                tid.emplace(b.ref_name, 0);
            else
                for (size_t i = 0; i < b.ctg->table->size(); ++i)
                    tid.emplace((*b.ctg->table)[i].name, (int64_t)i);
        }
        if (spool)
            return;
        if (bam) {
            if (b.header)
                bam->begin(b.path, header_text(b, "unsorted"));
            return;
        }
        out.open(b.path, b.header ? std::ios::out : std::ios::app);
        if (!out.is_open())
            throw Error(DRM_ERR_IO, "Failed to open SAM file: " + b.path);
        if (b.header)
            write_header(out, b, "unsorted");
    }
    void line(const SamLine &l)
    {
        if (!spool) {
            put(bam ? bam->pending() : buf, l);
            return;
        }
        int64_t t = -1;
        if (l.rname != "*") {
            const auto it = tid.find(l.rname);
            if (it == tid.end())
                throw Error(DRM_ERR_INTERNAL, "RNAME " + std::string(l.rname) + " is not in the header");
            t = it->second;
        }
        spool->keys.push_back(sam_sort_key(t, l.pos, (l.flag & 16) != 0));
        spool->offsets.push_back(spool->text.size());
        put(spool->text, l);
    }
    void end_record(bool last = false)
    {
        if (spool)
            return;
        if (bam) { // the tail is carried into the next block; the run's last bytes are BamSink::finish's
            bam->flush();
            return;
        }
        if (!last && buf.size() <= (1u << 22))
            return;
        out << buf;
        buf.clear();
    }
};

// the quality line of query g, empty without one
std::string_view qual_of(const SamBlock &b, size_t g)
{
    return b.quals && !b.quals->empty() ? std::string_view((*b.quals)[g]) : std::string_view();
}

} // namespace

// ----------------------------------------------------------------------- SAM (write_sam)
void drm::write_sam_block(const SamBlock &b, size_t nq, const int32_t *counts, size_t k, bool loci, bool xa)
{
    if (b.ctg && !b.aln)
        throw Error(DRM_ERR_ARG, "a contig table needs the rows' alignments");
    if ((loci && !b.aln) || (xa && !loci))
        throw Error(DRM_ERR_ARG, "lines per locus need the rows' alignments, and XA the lines per locus");
    const SamXa alternates{b.ids, counts, k, 1, b.aln, b.ctg};
    SamOut out(b);
    for (size_t i = 0; i < nq; ++i) {
        const size_t g = b.q0 + i;
        const std::string &tagged = (*b.queries)[g];
        // the reference's read: PREFIX "<" / POSTFIX ">" stripped (parse_inputs.hpp:10-11) whatever the ends hold
        const std::string_view whole = tagged, plain = whole.size() > 2 ? whole.substr(1, whole.size() - 2) : whole;
        const std::string qname = qname_of(b, g, g + 1);
        SamLine unmapped; // the read without a row: the line's other columns stay "*" and 0
        unmapped.qname = qname;
        const int dup = b.dup && b.dup[i] ? 1024 : 0; // DRM_SAM_DUP: on every line of the query
        unmapped.flag = 4 | dup;
        unmapped.read = plain;
        unmapped.qual = qual_of(b, g);
        // DRM_SAM_XA: the rows behind the primary go into its XA:Z tag
        const std::string xa_tail = xa && counts[i] > 1 ? xa_tag(alternates, i, tagged, b) : std::string();
        for (int j = 0; j < (xa ? std::min(counts[i], 1) : counts[i]) && (size_t)j < k; ++j) {
            const size_t row = i * k + (size_t)j;
            const uint64_t sid = b.ids[row];
            SamLine l = unmapped;
            l.flag = (j == 0 ? 0 : 256) | (sid % 2 == 1 ? 16 : 0) | dup; // primary / secondary, reverse complement
            Placed p; // real POS / CIGAR, SEQ on the forward strand; a hit without an alignment is written as unmapped
            if (b.aln) {
                p = place_row(b.aln, row, sid, tagged, b.ref_len, contig_of(b.ctg, row));
            } else { // the reference's pseudo fields: the window's start, the whole read matched, as read also under flag 16
                p.read = plain;
                p.mapped = true;
                p.pos1 = (int64_t)(sid / 2 + 1);
                p.cigar = std::to_string(plain.size()) + "M";
            }
            l.flag |= p.mapped ? 0 : 4;
            l.rname = p.contig ? p.contig->name : b.ref_name;
            l.pos = p.pos1;
            l.mapq = !b.mapq ? 60 : p.mapped ? b.mapq[row] : 0;
            l.cigar = p.cigar;
            l.read = p.read;
            l.reversed = p.reverse;
            if (b.aln && p.mapped)
                l.tags = mapped_tags(*b.aln, row, p.reverse, xa_tail);
            out.line(l);
        }
        // DRM_CONTIGS: a read without a row inside a contig is written unmapped; DRM_SAM_LOCI: a read without a locus
        if ((b.ctg || loci) && counts[i] < 1)
            out.line(unmapped);
        out.end_record();
    }
    out.end_record(true);
}

void drm::write_sam_pairs(const SamBlock &b, size_t npairs, const int32_t *counts, const int32_t *proper,
                          const SamXa *xa)
{
    const SamAlignments &aln = *b.aln;
    SamOut out(b);
    for (size_t pair = 0; pair < npairs; ++pair) {
        Placed p[2];
        drm_sam_mate in[2];
        drm_sam_mate_fields f[2];
        for (int m = 0; m < 2; ++m) {
            const size_t row = 2 * pair + (size_t)m;
            const std::string &tagged = (*b.queries)[b.q0 + row];
            // a read without a hit has no record, and one without an alignment may have no contig
            const bool hit = counts[row] >= 1 && aln.rec[row].status != 1;
            p[m] = place_row(hit ? &aln : nullptr, row, b.ids[row], tagged, b.ref_len, hit ? contig_of(b.ctg, row) : nullptr);
            in[m] = p[m].mapped ? drm_sam_mate{1, p[m].reverse, p[m].pos1, aln.rec[row].ref_end - aln.rec[row].ref_begin}
                                : drm_sam_mate{0, 0, 0, 0};
        }
        // DRM_CONTIGS: RNAME is the contig of the line's own position (an unmapped mate takes its mate's), RNEXT "=" on
        // one contig; mates on two contigs are never a proper pair and have no template length
        const std::string *rname[2] = {&b.ref_name, &b.ref_name};
        for (int m = 0; m < 2; ++m)
            if (const FastaContig *c = p[p[m].mapped ? m : 1 - m].contig)
                rname[m] = &c->name;
        const bool split = p[0].mapped && p[1].mapped && p[0].contig != p[1].contig;
        sam_pair_fields(in, proper[pair] != 0 && !split, f);
        if (split)
            f[0].tlen = f[1].tlen = 0;
        const std::string qname = qname_of(b, b.q0 + 2 * pair, (b.q0 + 2 * pair) / 2 + 1);
        for (int m = 0; m < 2; ++m) {
            const size_t row = 2 * pair + (size_t)m;
            SamLine l;
            l.qname = qname;
            l.flag = f[m].flag | (b.dup && b.dup[row] ? 1024 : 0); // DRM_SAM_DUP: the pair's answer on both lines
            if (f[m].has_rname) {
                l.rname = *rname[m];
                l.rnext = split ? std::string_view(*rname[1 - m]) : std::string_view("=");
            }
            l.pos = f[m].pos;
            l.mapq = !b.mapq ? 60 : p[m].mapped ? b.mapq[row] : 0;
            l.cigar = p[m].cigar;
            l.pnext = f[m].pnext;
            l.tlen = f[m].tlen;
            l.read = p[m].read;
            l.qual = qual_of(b, b.q0 + row);
            l.reversed = p[m].reverse;
            if (p[m].mapped) // DRM_SAM_LOCI: the mate's other loci behind its own tags
                l.tags = mapped_tags(aln, row, p[m].reverse,
                                     xa ? xa_tag(*xa, row, (*b.queries)[b.q0 + row], b) : std::string());
            out.line(l);
        }
        out.end_record();
    }
    out.end_record(true);
}

// ----------------------------------------------------------------------- the coordinate-sorted file
extern "C" int drm_sam_sort_key(int64_t tid, int64_t pos, int32_t reverse, uint64_t *key)
{
    return drm::guarded([&] {
        if (!key)
            throw Error(DRM_ERR_ARG, "null argument");
        *key = sam_sort_key(tid, pos, reverse != 0);
    });
}

void drm::write_sam_sorted(const SamBlock &b, const SamSpool &spool, const uint32_t *order)
{
    const size_t n = spool.keys.size();
    if (spool.offsets.size() != n || (n > 0 && !order))
        throw Error(DRM_ERR_ARG, "the spool's lines, keys and order do not match");
    // written beside the file and renamed when complete: a run that fails here leaves no half-sorted results
    const std::string part = b.path + ".part";
    try {
        std::ofstream out(part, std::ios::out | std::ios::trunc);
        if (!out.is_open())
            throw Error(DRM_ERR_IO, "Failed to open SAM file: " + part);
        write_header(out, b, "coordinate");
        std::string buf;
        for (size_t i = 0; i < n; ++i) {
            const size_t l = order[i];
            if (l >= n)
                throw Error(DRM_ERR_INTERNAL, "order[" + std::to_string(i) + "] = " + std::to_string(l) + " of " +
                                                  std::to_string(n) + " lines");
            const size_t from = spool.offsets[l], to = l + 1 < n ? spool.offsets[l + 1] : spool.text.size();
            buf.append(spool.text, from, to - from);
            if (buf.size() > (1u << 22)) {
                out << buf;
                buf.clear();
            }
        }
        out << buf;
        out.close();
        if (!out)
            throw Error(DRM_ERR_IO, "Failed to write SAM file: " + part);
        if (std::rename(part.c_str(), b.path.c_str()) != 0)
            throw Error(DRM_ERR_IO, "Failed to rename " + part + " to " + b.path);
    } catch (...) {
        std::remove(part.c_str());
        throw;
    }
}

void drm::write_bam_sorted(const SamBlock &b, const SamSpool &spool, const uint32_t *order)
{
    const size_t n = spool.keys.size();
    if (spool.offsets.size() != n || (n > 0 && !order) || !b.bam)
        throw Error(DRM_ERR_ARG, "the spool's records, keys and order do not match, or there is no BAM sink");
    // written beside the file and renamed when complete, as write_sam_sorted does
    const std::string part = b.path + ".part";
    try {
        b.bam->begin(part, header_text(b, "coordinate"));
        for (size_t i = 0; i < n; ++i) {
            const size_t l = order[i];
            if (l >= n)
                throw Error(DRM_ERR_INTERNAL, "order[" + std::to_string(i) + "] = " + std::to_string(l) + " of " +
                                                  std::to_string(n) + " records");
            const size_t from = spool.offsets[l], to = l + 1 < n ? spool.offsets[l + 1] : spool.text.size();
            b.bam->pending().append(spool.text, from, to - from);
            b.bam->flush();
        }
        b.bam->finish();
        if (std::rename(part.c_str(), b.path.c_str()) != 0)
            throw Error(DRM_ERR_IO, "Failed to rename " + part + " to " + b.path);
    } catch (...) {
        std::remove(part.c_str());
        throw;
    }
}
