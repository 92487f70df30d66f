// tests/sam_sort_driver.cpp -- the spool and the final writer of DRM_SAM_SORT=coordinate on the CPU
// (tests/test_sam_sort_writer_cpu.py). The blocks are sam_writer_driver.cpp's, whose text is included here with its main
// renamed. Every case is written twice into <output directory>: <case>.unsorted.sam by the writers as they are, and
// <case>.sorted.sam through a SamSpool, a std::stable_sort of the spool's keys and write_sam_sorted. The GPU sort is not
// part of this program: it is compiled with AddressSanitizer and UBSan and runs anywhere.
#define main sam_writer_driver_main
#include "sam_writer_driver.cpp"
#undef main

#include <numeric>

namespace {

std::vector<uint32_t> stable_order(const drm::SamSpool &s)
{
    std::vector<uint32_t> order(s.keys.size());
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return s.keys[a] < s.keys[b]; });
    return order;
}

void write_sorted(const std::string &path, const drm::SamSpool &s, const Mode &m, const uint32_t *order)
{
    const drm::SamContigs sc{&kContigs, nullptr};
    drm::SamBlock b;
    b.path = path;
    b.ref_len = kRefLen;
    b.ctg = m.contigs ? &sc : nullptr;
    drm::write_sam_sorted(b, s, order);
}

void sorted_reads(const std::string &dir, const std::string &name, const Reads &r, const std::vector<ReadBlock> &blocks,
                  const Mode &m)
{
    drm::SamSpool spool;
    for (size_t x = 0; x < blocks.size(); ++x) {
        const ReadBlock &b = blocks[x];
        write_reads(dir + "/" + name + ".unsorted.sam", x == 0, r, b, m);
        const Flat f(b.rows);
        const drm::SamAlignments av = view(f, m);
        const drm::SamContigs sc{&kContigs, f.contig.data()};
        drm::SamBlock sb = block("/nonexistent/never_opened.sam", x == 0, r, b.q0, f, m, kRefLen, &av, &sc, b.dup);
        sb.spool = &spool;
        drm::write_sam_block(sb, b.nq, b.counts.data(), b.k, m.loci, m.xa);
    }
    const std::vector<uint32_t> order = stable_order(spool);
    write_sorted(dir + "/" + name + ".sorted.sam", spool, m, order.data());
}

void sorted_pairs(const std::string &dir, const std::string &name, const std::vector<PairBlock> &blocks, const Mode &m)
{
    const Reads r = pair_reads();
    drm::SamSpool spool;
    for (size_t x = 0; x < blocks.size(); ++x) {
        const PairBlock &b = blocks[x];
        write_pairs(dir + "/" + name + ".unsorted.sam", x == 0, r, b, m);
        const Flat f(b.rows), xf(b.xa_rows);
        const drm::SamAlignments av = view(f, m), xav = view(xf, m);
        const drm::SamContigs sc{&kContigs, f.contig.data()}, xsc{&kContigs, xf.contig.data()};
        const drm::SamXa xa{xf.ids.data(), b.xa_counts.data(), b.xa_width, 0, &xav, m.contigs ? &xsc : nullptr};
        drm::SamBlock sb = block("/nonexistent/never_opened.sam", x == 0, r, b.q0, f, m, kRefLen, &av, &sc, b.dup);
        sb.spool = &spool;
        drm::write_sam_pairs(sb, b.npairs, b.counts.data(), b.proper.data(), m.xa ? &xa : nullptr);
    }
    const std::vector<uint32_t> order = stable_order(spool);
    write_sorted(dir + "/" + name + ".sorted.sam", spool, m, order.data());
}

// a spool of 15 MB, past the final writer's 4 MiB flush three times, the reads spread over 5000 positions of two contigs
void sorted_flush(const std::string &dir)
{
    Reads r;
    ReadBlock b;
    big_reads(40000, r, b);
    for (size_t i = 0; i < b.rows.size(); ++i) {
        b.rows[i].region_start -= (int64_t)(i * 7919 % 5000);
        b.rows[i].contig = (int32_t)(i % 3 == 0);
        b.rows[i].id ^= (uint64_t)(i % 5 == 0);
    }
    Mode m;
    m.aln = m.region = m.md = m.contigs = m.quals = m.mapq = true;
    sorted_reads(dir, "flush", r, {b}, m);
}

bool exists(const std::string &path) { return std::ifstream(path).good(); }

// what write_sam_sorted refuses, and what it leaves behind then: nothing
int errors(const std::string &dir)
{
    drm::SamSpool s;
    s.text = "a\nb\n";
    s.offsets = {0, 2};
    s.keys = {5, 3};
    Mode m;
    int bad = 0;
    auto refused = [&](const char *what, const std::string &path, const drm::SamSpool &sp, const uint32_t *order, int code) {
        try {
            write_sorted(path, sp, m, order);
            std::fprintf(stderr, "sam_sort_driver: %s was accepted\n", what);
            ++bad;
        } catch (const drm::Error &e) {
            if (e.code != code || exists(path) || exists(path + ".part")) {
                std::fprintf(stderr, "sam_sort_driver: %s: code %d, or a file was left behind\n", what, e.code);
                ++bad;
            }
        }
    };
    const uint32_t past[2] = {1, 2}, fine[2] = {1, 0};
    refused("an index past the spool", dir + "/err_past.sam", s, past, DRM_ERR_INTERNAL);
    refused("a null order", dir + "/err_null.sam", s, nullptr, DRM_ERR_ARG);
    drm::SamSpool uneven = s;
    uneven.keys.push_back(1);
    refused("keys without lines", dir + "/err_uneven.sam", uneven, fine, DRM_ERR_ARG);
    refused("a directory that does not exist", dir + "/missing/err.sam", s, fine, DRM_ERR_IO);
    write_sorted(dir + "/two_lines.sorted.sam", s, m, fine);
    write_sorted(dir + "/empty.sorted.sam", drm::SamSpool(), m, nullptr);
    return bad;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s <output directory>\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    try {
        Mode m;
        m.aln = m.quals = m.mapq = true;
        sorted_reads(dir, "aligned", six_reads(), aligned_blocks(), m);
        m.contigs = true;
        sorted_reads(dir, "contigs", six_reads(), contig_blocks(aligned_blocks()), m);
        m = Mode();
        m.aln = m.loci = m.quals = m.region = m.contigs = m.md = m.mapq = true;
        sorted_reads(dir, "loci", six_reads(), loci_blocks(), m);
        sorted_reads(dir, "loci_dup", six_reads(), loci_dup_blocks(), m);
        m.xa = true;
        sorted_reads(dir, "loci_xa", six_reads(), loci_blocks(), m);
        m = Mode();
        m.aln = m.quals = true;
        sorted_pairs(dir, "pairs", pair_blocks(), m);
        sorted_pairs(dir, "pairs_dup", pair_dup_blocks(), m);
        m.mapq = m.contigs = true;
        sorted_pairs(dir, "pairs_contigs", pair_contig_blocks(pair_blocks()), m);
        m.xa = m.region = true;
        sorted_pairs(dir, "pairs_xa", pair_xa_blocks(pair_contig_blocks(pair_blocks())), m);
        sorted_flush(dir);
        if (errors(dir))
            return 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "sam_sort_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
