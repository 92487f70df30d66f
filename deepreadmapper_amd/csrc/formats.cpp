// deepreadmapper_amd/csrc/formats.cpp -- host-side formats of the reference path.
//   config.txt   save_config / load_config      src/utils/utils.cpp:505-597
//   .npy         cnpy::npy_save / npy_load       src/utils/utils.cpp:284-285, src/main.cpp:109
//   FASTA        format_fasta (+ reverse_complement) src/utils/parse_inputs.cpp:43-53, :223-369
//   FASTQ        format_fastq                    src/utils/parse_inputs.cpp:843-950
//   .txt         read_txt_mmap                   src/utils/utils.cpp:94-186
#include <array>
#include <cctype>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <sstream>
#include <unordered_set>

#include "drm_internal.h"

namespace drm {

// ------------------------------------------------------------------------------ config.txt
void save_config(const std::unordered_map<std::string, ConfigValue> &config, const std::string &folder,
                 const std::string &file)
{
    std::filesystem::create_directories(folder);
    std::string path = folder + "/" + file;
    std::ofstream out(path);
    if (!out)
        throw Error(DRM_ERR_IO, "Could not create config file: " + file);
    // unordered_map iteration order, exactly as utils.cpp:517-533 emits it
    for (const auto &kv : config) {
        out << kv.first << ": ";
        if (std::holds_alternative<size_t>(kv.second))
            out << std::get<size_t>(kv.second);
        else if (std::holds_alternative<float>(kv.second))
            out << std::get<float>(kv.second);
        else
            out << std::get<std::string>(kv.second);
        out << "\n";
    }
}

std::unordered_map<std::string, ConfigValue> load_config(const std::string &path)
{
    std::ifstream in(path);
    if (!in)
        throw Error(DRM_ERR_IO, "Could not open config file: " + path);
    std::unordered_map<std::string, ConfigValue> config;
    std::string line;
    while (std::getline(in, line)) {
        size_t delim = line.find(':');
        if (delim == std::string::npos)
            continue;
        std::string key = line.substr(0, delim);
        std::string val = line.substr(delim + 1);
        key.erase(0, key.find_first_not_of(" \t"));
        key.erase(key.find_last_not_of(" \t") + 1);
        val.erase(0, val.find_first_not_of(" \t"));
        val.erase(val.find_last_not_of(" \t") + 1);
        // size_t, then float, else string (utils.cpp:565-592)
        try {
            size_t idx;
            size_t v = std::stoull(val, &idx);
            if (idx == val.size()) {
                config[key] = v;
                continue;
            }
        } catch (...) {
        }
        try {
            size_t idx;
            float v = std::stof(val, &idx);
            if (idx == val.size()) {
                config[key] = v;
                continue;
            }
        } catch (...) {
        }
        config[key] = val;
    }
    return config;
}

// ------------------------------------------------------------------------------ npy (cnpy layout)
void npy_save(const std::string &path, const void *data, const std::vector<size_t> &shape, char kind, int itemsize)
{
    std::string dict = "{'descr': '<";
    dict += kind;
    dict += std::to_string(itemsize);
    dict += "', 'fortran_order': False, 'shape': (";
    dict += std::to_string(shape.empty() ? 0 : shape[0]);
    for (size_t i = 1; i < shape.size(); i++) {
        dict += ", ";
        dict += std::to_string(shape[i]);
    }
    if (shape.size() == 1)
        dict += ",";
    dict += "), }";
    int remainder = 16 - (10 + (int)dict.size()) % 16; // cnpy pads even when already aligned
    dict.append((size_t)remainder, ' ');
    dict.back() = '\n';
    std::string header;
    header += (char)0x93;
    header += "NUMPY";
    header += (char)0x01;
    header += (char)0x00;
    uint16_t hl = (uint16_t)dict.size();
    header.append((const char *)&hl, 2);
    header += dict;
    size_t nel = 1;
    for (size_t s : shape)
        nel *= s;
    std::FILE *f = std::fopen(path.c_str(), "wb");
    if (!f)
        throw Error(DRM_ERR_IO, "Could not create file: " + path);
    std::fwrite(header.data(), 1, header.size(), f);
    if (nel)
        std::fwrite(data, (size_t)itemsize, nel, f);
    std::fclose(f);
}

NpyArray npy_load(const std::string &path)
{
    std::string s = read_whole_file(path);
    if (s.size() < 10 || (unsigned char)s[0] != 0x93 || s.compare(1, 5, "NUMPY") != 0)
        throw Error(DRM_ERR_FORMAT, "not a .npy file: " + path);
    int major = (unsigned char)s[6];
    size_t hl, off;
    if (major == 1) {
        hl = (unsigned char)s[8] | ((unsigned char)s[9] << 8);
        off = 10;
    } else {
        if (s.size() < 12)
            throw Error(DRM_ERR_FORMAT, "truncated .npy: " + path);
        hl = (unsigned char)s[8] | ((unsigned char)s[9] << 8) | ((unsigned char)s[10] << 16) |
             ((size_t)(unsigned char)s[11] << 24);
        off = 12;
    }
    if (off + hl > s.size())
        throw Error(DRM_ERR_FORMAT, "truncated .npy header: " + path);
    std::string h = s.substr(off, hl);
    NpyArray a;
    size_t p = h.find("'descr'");
    size_t q1 = h.find('\'', h.find(':', p) + 1);
    size_t q2 = h.find('\'', q1 + 1);
    std::string descr = h.substr(q1 + 1, q2 - q1 - 1);
    if (descr.size() < 3 || (descr[0] != '<' && descr[0] != '|'))
        throw Error(DRM_ERR_FORMAT, "unsupported npy descr " + descr);
    a.kind = descr[1];
    a.itemsize = std::stoi(descr.substr(2));
    a.fortran = h.find("'fortran_order': True") != std::string::npos;
    size_t sp = h.find('(', h.find("'shape'"));
    size_t se = h.find(')', sp);
    std::string shp = h.substr(sp + 1, se - sp - 1);
    std::stringstream ss(shp);
    std::string tok;
    while (std::getline(ss, tok, ',')) {
        tok.erase(0, tok.find_first_not_of(" "));
        tok.erase(tok.find_last_not_of(" ") + 1);
        if (!tok.empty())
            a.shape.push_back(std::stoull(tok));
    }
    size_t nel = 1;
    for (size_t d : a.shape)
        nel *= d;
    size_t need = nel * (size_t)a.itemsize;
    if (off + hl + need > s.size())
        throw Error(DRM_ERR_FORMAT, "truncated .npy data: " + path);
    a.bytes.assign(s.begin() + off + hl, s.begin() + off + hl + need);
    return a;
}

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

std::string reverse_complement(const std::string &seq)
{
    const auto &t = comp_table();
    std::string rc;
    rc.reserve(seq.size());
    for (auto it = seq.rbegin(); it != seq.rend(); ++it) {
        unsigned char c = (unsigned char)*it;
        rc.push_back(c < 128 ? t[c] : '\0');
    }
    return rc;
}

std::vector<std::string> format_fasta(const std::string &data, size_t ref_len, size_t stride, bool lookup_mode)
{
    // Step 1 (:233-272): contigs = ACGTN letters (upper-cased) after each '>' header line
    std::vector<std::string> contigs;
    std::string cur;
    bool in_seq = false;
    size_t i = 0, n = data.size();
    while (i < n) {
        if (data[i] == '>') {
            if (!cur.empty()) {
                contigs.push_back(std::move(cur));
                cur.clear();
            }
            while (i < n && data[i] != '\n')
                i++;
            if (i < n)
                i++;
            in_seq = true;
            continue;
        }
        if (in_seq) {
            char c = data[i];
            if (!std::isspace((unsigned char)c)) {
                c = (char)std::toupper((unsigned char)c);
                if (c == 'A' || c == 'T' || c == 'C' || c == 'G' || c == 'N')
                    cur.push_back(c);
            }
        }
        i++;
    }
    if (!cur.empty())
        contigs.push_back(std::move(cur));
    // Step 4 (:325-362): per contig, window i at i*stride, forward then reverse complement
    std::vector<std::string> out;
    for (const auto &seq : contigs) {
        if (seq.size() < ref_len)
            continue;
        size_t nw = (seq.size() - ref_len) / stride + 1;
        for (size_t w = 0; w < nw; ++w) {
            std::string win = seq.substr(w * stride, ref_len);
            std::string rev = reverse_complement(win);
            if (!lookup_mode) {
                out.push_back("<" + win + ">");
                out.push_back("<" + rev + ">");
            } else {
                out.push_back(win);
                out.push_back(rev);
            }
        }
    }
    return out;
}

void format_fastq(const std::string &data, std::vector<std::string> &seqs, std::vector<std::string> &ids)
{
    const char *cur = data.data();
    const char *end = cur + data.size();
    int line = 0;
    while (cur < end) {
        const char *ls = cur;
        while (cur < end && *cur != '\n')
            cur++;
        if (line % 4 == 0) {
            const char *hs = ls;
            if (hs < cur && *hs == '@')
                hs++;
            const char *ie = hs;
            while (ie < cur && *ie != ' ' && *ie != '\t' && *ie != '/')
                ie++;
            ids.emplace_back(hs, ie - hs);
        } else if (line % 4 == 1) {
            std::string s;
            s.reserve((size_t)(cur - ls) + 2);
            s += '<';
            s.append(ls, cur - ls);
            s += '>';
            seqs.push_back(std::move(s));
        }
        if (cur < end)
            cur++;
        line++;
    }
}

void format_fastq_qual(const std::string &data, std::vector<std::string> &seqs, std::vector<std::string> &ids,
                       std::vector<std::string> &quals)
{
    format_fastq(data, seqs, ids);
    // the same line walk: line 4 r + 3 belongs to record r
    const char *cur = data.data();
    const char *end = cur + data.size();
    for (int line = 0; cur < end; ++line) {
        const char *ls = cur;
        while (cur < end && *cur != '\n')
            cur++;
        if (line % 4 == 3)
            quals.emplace_back(ls, cur - ls);
        if (cur < end)
            cur++;
    }
    quals.resize(seqs.size()); // a last record cut off before its quality line fails the length check below
    for (size_t r = 0; r < seqs.size(); ++r)
        if (quals[r].size() + 2 != seqs[r].size())
            throw Error(DRM_ERR_FORMAT, "read " + std::to_string(r) + " (" + (r < ids.size() ? ids[r] : std::string()) +
                                            ") has " + std::to_string(seqs[r].size() - 2) + " bases and " +
                                            std::to_string(quals[r].size()) + " quality characters");
}

void read_file_qual(const std::string &path, std::vector<std::string> &seqs, std::vector<std::string> &ids,
                    std::vector<std::string> &quals)
{
    const std::string ext = std::filesystem::path(path).extension().string();
    quals.clear();
    if (ext != ".fastq" && ext != ".fq") {
        read_file(path, seqs, ids);
        return;
    }
    const std::string data = read_whole_file(path);
    seqs.clear();
    ids.clear();
    format_fastq_qual(data, seqs, ids, quals);
}

void read_file(const std::string &path, std::vector<std::string> &seqs, std::vector<std::string> &ids,
               size_t ref_len, size_t stride, bool lookup_mode)
{
    std::string ext = std::filesystem::path(path).extension().string();
    if (ext != ".fna" && ext != ".fasta" && ext != ".fa" && ext != ".fastq" && ext != ".fq" && ext != ".txt")
        throw Error(DRM_ERR_ARG, "Unsupported file format: " + ext + ". Only .fna/.fastq/.txt are supported.");
    std::string data = read_whole_file(path);
    seqs.clear();
    ids.clear();
    if (ext == ".fna" || ext == ".fasta" || ext == ".fa") {
        seqs = format_fasta(data, ref_len, stride, lookup_mode);
        return;
    }
    if (ext == ".fastq" || ext == ".fq") {
        format_fastq(data, seqs, ids);
        return;
    }
    // read_txt_mmap (utils.cpp:140-165): non-empty lines, split on '\n' / '\r'
    const char *c = data.data(), *e = c + data.size();
    while (c < e) {
        const char *ls = c;
        while (c < e && *c != '\n' && *c != '\r')
            c++;
        if (c > ls)
            seqs.emplace_back(ls, c - ls);
        while (c < e && (*c == '\n' || *c == '\r'))
            c++;
    }
}

} // namespace drm

// ----------------------------------------------------------------------- extract_FASTA_sequence
std::string drm::extract_fasta_sequence(const std::string &path)
{
    const std::string data = read_whole_file(path);
    size_t p = data.find('\n');
    p = p == std::string::npos ? data.size() : p + 1; // skip the first (header) line
    std::string g;
    g.reserve(data.size() - p);
    for (; p < data.size(); ++p) {
        const unsigned char c = (unsigned char)data[p];
        if (std::isspace(c))
            continue;
        const char u = (char)std::toupper(c);
        if (u == 'A' || u == 'T' || u == 'C' || u == 'G' || u == 'N')
            g.push_back(u);
    }
    return g;
}

// ----------------------------------------------------------------------- contig table of a FASTA
std::vector<drm::FastaContig> drm::fasta_contigs(const std::string &path)
{
    const std::string data = read_whole_file(path);
    std::vector<FastaContig> out;
    std::unordered_set<std::string> seen;
    int64_t glen = 0; // the length of extract_fasta_sequence's string so far
    auto label = [&]() {
        return "contig " + std::to_string(out.size() - 1) + " (\"" + out.back().name + "\")";
    };
    auto close = [&]() { // the open contig ends at glen
        out.back().len = glen - out.back().start;
        if (out.back().len == 0)
            throw Error(DRM_ERR_FORMAT, path + ": " + label() + " has no sequence");
    };
    auto is_base = [](unsigned char c) {
        const int u = std::toupper(c);
        return u == 'A' || u == 'T' || u == 'C' || u == 'G' || u == 'N';
    };
    if (data.empty() || data[0] != '>')
        throw Error(DRM_ERR_FORMAT, path + ": the first line does not start with '>' (the header of contig 0)");
    for (size_t p = 0; p < data.size();) {
        size_t e = data.find('\n', p);
        e = e == std::string::npos ? data.size() : e;
        if (data[p] == '>') {
            if (!out.empty()) {
                close();
                for (size_t i = p; i < e; ++i) // a later header's letters are a gap in the string
                    glen += is_base((unsigned char)data[i]);
            }
            size_t q = p + 1;
            while (q < e && !std::isspace((unsigned char)data[q]))
                ++q;
            FastaContig c;
            c.name = data.substr(p + 1, q - p - 1);
            c.start = glen;
            if (c.name.empty())
                throw Error(DRM_ERR_FORMAT, path + ": contig " + std::to_string(out.size()) + " has an empty name");
            if (!seen.insert(c.name).second)
                throw Error(DRM_ERR_FORMAT, path + ": contig " + std::to_string(out.size()) + " repeats the name \"" +
                                                c.name + "\"");
            out.push_back(std::move(c));
        } else {
            for (size_t i = p; i < e; ++i) {
                const unsigned char c = (unsigned char)data[i];
                if (std::isspace(c))
                    continue;
                if (!is_base(c))
                    throw Error(DRM_ERR_FORMAT, path + ": " + label() + " holds the byte '" + std::string(1, (char)c) +
                                                    "' at base " + std::to_string(glen - out.back().start) +
                                                    ": only A, C, G, T and N are kept, so it would shift every later "
                                                    "coordinate");
                ++glen;
            }
        }
        p = e + 1;
    }
    close();
    return out;
}

extern "C" int drm_fasta_contigs(const char *path, int64_t *n, int64_t *starts, int64_t *lens, char *names,
                                 int64_t *names_bytes)
{
    try {
        if (!path || !n || !names_bytes)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        const std::vector<drm::FastaContig> t = drm::fasta_contigs(path);
        int64_t bytes = 0;
        for (const drm::FastaContig &c : t)
            bytes += (int64_t)c.name.size() + 1;
        if (starts) {
            if (*n < (int64_t)t.size() || (names && *names_bytes < bytes))
                throw drm::Error(DRM_ERR_ARG, "the arrays are too small for " + std::to_string(t.size()) +
                                                  " contigs and " + std::to_string(bytes) + " bytes of names");
            char *w = names;
            for (size_t i = 0; i < t.size(); ++i) {
                starts[i] = t[i].start;
                if (lens)
                    lens[i] = t[i].len;
                if (names) {
                    std::memcpy(w, t[i].name.c_str(), t[i].name.size() + 1);
                    w += t[i].name.size() + 1;
                }
            }
        }
        *n = (int64_t)t.size();
        *names_bytes = bytes;
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_IO;
    }
}

// ----------------------------------------------------------------------- SAM from a GPU alignment
// CIGAR + POS of one drm_sw_alignment record over the region genome[region_start ..+ region_len), reverse-complemented
// when rev (include/drm_hip.h: drm_sam_cigar_region; drm_sam_cigar is the region of a window id)
static void sam_cigar(const drm_sw_alignment &a, const uint32_t *ops, int32_t q_len, int32_t tag_prefix,
                      int32_t tag_postfix, int64_t region_start, int32_t region_len, bool rev, int64_t &pos1,
                      std::string &cigar)
{
    using drm::Error;
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
    try {
        if (!a || !pos1 || !cigar)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        std::string c;
        int64_t p = 0;
        sam_cigar(*a, ops, q_len, tag_prefix, tag_postfix, region_start, region_len, reverse != 0, p, c);
        if ((int64_t)c.size() + 1 > (int64_t)cigar_cap)
            throw drm::Error(DRM_ERR_ARG, "cigar_cap " + std::to_string(cigar_cap) + " is too small for " +
                                              std::to_string(c.size() + 1) + " bytes");
        std::memcpy(cigar, c.c_str(), c.size() + 1);
        *pos1 = p;
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_ARG;
    }
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
    using drm::Error;
    if (h.status != 0)
        throw Error(DRM_ERR_ARG, h.status == 2 ? "the record's MD words are truncated (status 2): compute the pair again "
                                                 "with a larger md_stride"
                                               : "the record holds no MD words (status " + std::to_string(h.status) + ")");
    if (h.n_words < 1 || !words)
        throw Error(DRM_ERR_ARG, "an MD stream holds at least one number");
    const auto &comp = drm::comp_table();
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
    try {
        if (!h || !md)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        std::string s;
        sam_md(*h, words, reverse != 0, s);
        if ((int64_t)s.size() + 1 > (int64_t)md_cap)
            throw drm::Error(DRM_ERR_ARG, "md_cap " + std::to_string(md_cap) + " is too small for " +
                                              std::to_string(s.size() + 1) + " bytes");
        std::memcpy(md, s.c_str(), s.size() + 1);
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_ARG;
    }
}

// DRM_SAM_MD: "\tMD:Z:<string>" of a mapped row, nothing when the block carries no MD records
static void append_md_tag(std::string &buf, const drm::SamAlignments &aln, size_t row, bool rev)
{
    if (!aln.md)
        return;
    std::string md;
    sam_md(aln.md[row], aln.md_words + aln.md_off[row], rev, md);
    buf += "\tMD:Z:" + md;
}

// DRM_SAM_LOCI: "\tXA:Z:" and one "RNAME,<+|->POS,CIGAR,NM;" per alternate of block row `read` that holds an
// alignment; empty when none does (drm_internal.h, SamXa)
static std::string xa_tag(const drm::SamXa &xa, size_t read, const std::string &tagged, const std::string &ref_name,
                          size_t ref_len)
{
    const int pre = !tagged.empty() && tagged.front() == '<', post = tagged.size() > 1 && tagged.back() == '>';
    const drm::SamAlignments &aln = *xa.aln;
    std::string tag, cigar;
    for (size_t j = xa.first; j < xa.width && (int64_t)j < (int64_t)xa.counts[read]; ++j) {
        const size_t row = read * xa.width + j;
        const drm_sw_alignment &a = aln.rec[row];
        if (a.status == 1)
            continue;
        const uint64_t sid = xa.ids[row];
        const bool rev = (sid & 1u) != 0;
        int64_t pos1 = 0;
        if (aln.region_start)
            sam_cigar(a, aln.ops + aln.ops_off[row], (int32_t)tagged.size(), pre, post, aln.region_start[row],
                      aln.region_len[row], rev, pos1, cigar);
        else
            sam_cigar(a, aln.ops + aln.ops_off[row], (int32_t)tagged.size(), pre, post, (int64_t)(sid / 2),
                      (int32_t)ref_len, rev, pos1, cigar);
        const drm::FastaContig *c = xa.ctg ? &(*xa.ctg->table)[(size_t)xa.ctg->row_contig[row]] : nullptr;
        tag += tag.empty() ? "\tXA:Z:" : "";
        tag += (c ? c->name : ref_name) + "," + (rev ? "-" : "+") + std::to_string(pos1 - (c ? c->start : 0)) + "," +
               cigar + "," + std::to_string(a.nm) + ";";
    }
    return tag;
}

// one row of the DRM_SAM_CIGAR mode: real POS / CIGAR, SEQ on the forward strand, AS and NM; a hit without an
// alignment is written as unmapped. `tail` (the XA:Z tag) comes last on a mapped line.
static void append_aligned_row(std::string &buf, const std::string &qname, int flag, const std::string &ref_name,
                               size_t ref_len, const std::string &tagged, uint64_t sid,
                               const drm::SamAlignments &aln, size_t row, const int32_t *mapq, int64_t contig_start = 0,
                               const std::string *qual = nullptr, const std::string *tail = nullptr)
{
    const drm_sw_alignment &a = aln.rec[row];
    // the read is the query without format_fastq's tags (an untagged .txt query is the read itself)
    const int pre = !tagged.empty() && tagged.front() == '<', post = tagged.size() > 1 && tagged.back() == '>';
    const std::string clean = tagged.substr((size_t)pre, tagged.size() - (size_t)pre - (size_t)post);
    std::string cigar = "*";
    int64_t pos1 = 0;
    if (a.status == 1)
        flag |= 4;
    else if (aln.region_start) // aligned over a flanked region (drm_sw_align_affine)
        sam_cigar(a, aln.ops + aln.ops_off[row], (int32_t)tagged.size(), pre, post, aln.region_start[row],
                  aln.region_len[row], (sid & 1u) != 0, pos1, cigar);
    else
        sam_cigar(a, aln.ops + aln.ops_off[row], (int32_t)tagged.size(), pre, post, (int64_t)(sid / 2), (int32_t)ref_len,
                  (sid & 1u) != 0, pos1, cigar);
    buf += qname;
    buf += '\t';
    buf += std::to_string(flag);
    buf += '\t';
    buf += ref_name;
    buf += '\t';
    buf += std::to_string(a.status == 1 ? pos1 : pos1 - contig_start); // DRM_CONTIGS: the contig's own coordinate
    buf += '\t';
    buf += mapq ? std::to_string(a.status == 1 ? 0 : mapq[row]) : std::string("60");
    buf += '\t';
    buf += cigar;
    buf += "\t*\t0\t0\t";
    buf += clean.empty() ? std::string("*") : (flag & 16) ? drm::reverse_complement(clean) : clean;
    buf += '\t';
    buf += !qual || qual->empty() ? std::string("*") : (flag & 16) ? std::string(qual->rbegin(), qual->rend()) : *qual;
    if (a.status != 1) {
        buf += "\tAS:i:" + std::to_string(a.score);
        buf += "\tNM:i:" + std::to_string(a.nm);
        append_md_tag(buf, aln, row, (sid & 1u) != 0);
        if (tail)
            buf += *tail;
    }
    buf += '\n';
}

// @HD, then @SQ: the reference's one line, or with a contig table (DRM_CONTIGS) one line per contig in file order
static void sam_header(std::ofstream &out, const std::string &ref_name, size_t ref_len, const drm::SamContigs *ctg)
{
    out << "@HD\tVN:1.0\tSO:unsorted\n";
    if (!ctg) {
        out << "@SQ\tSN:" << ref_name << "\tLN:" << ref_len << "\n";
        return;
    }
    for (const drm::FastaContig &c : *ctg->table)
        out << "@SQ\tSN:" << c.name << "\tLN:" << c.len << "\n";
}

// ----------------------------------------------------------------------- SAM (write_sam)
void drm::write_sam_block(const std::string &path, bool header, const std::string &ref_name, size_t ref_len,
                          const std::vector<std::string> &query_seqs, const std::vector<std::string> &query_ids,
                          size_t q0, size_t nq, const uint64_t *ids, const int32_t *counts, size_t k,
                          const SamAlignments *aln, const int32_t *mapq, const SamContigs *ctg,
                          const std::vector<std::string> *quals, bool loci, bool xa)
{
    if (quals && quals->empty())
        quals = nullptr;
    if (ctg && !aln)
        throw Error(DRM_ERR_ARG, "a contig table needs the rows' alignments");
    if ((loci && !aln) || (xa && !loci))
        throw Error(DRM_ERR_ARG, "lines per locus need the rows' alignments, and XA the lines per locus");
    const SamXa alternates{ids, counts, k, 1, aln, ctg};
    std::ofstream out(path, header ? std::ios::out : std::ios::app);
    if (!out.is_open())
        throw Error(DRM_ERR_IO, "Failed to open SAM file: " + path);
    if (header)
        sam_header(out, ref_name, ref_len, ctg);
    std::string buf;
    for (size_t i = 0; i < nq; ++i) {
        const size_t g = q0 + i;
        std::string clean = query_seqs[g]; // PREFIX "<" / POSTFIX ">" stripped (parse_inputs.hpp:10-11)
        if (clean.size() > 2)
            clean = clean.substr(1, clean.size() - 2);
        const std::string qname = (g < query_ids.size() && !query_ids[g].empty()) ? query_ids[g]
                                                                                  : "S1/" + std::to_string(g + 1) + "/0";
        const std::string cigar = std::to_string(clean.size()) + "M";
        const std::string *qual = quals ? &(*quals)[g] : nullptr;
        const std::string qual_col = qual && !qual->empty() ? *qual : std::string("*");
        // DRM_SAM_XA: the rows behind the primary go into its XA:Z tag
        const std::string tail = xa && counts[i] > 1 ? xa_tag(alternates, i, query_seqs[g], ref_name, ref_len)
                                                     : std::string();
        for (int j = 0; j < (xa ? std::min(counts[i], 1) : counts[i]) && (size_t)j < k; ++j) {
            const uint64_t sid = ids[i * k + (size_t)j];
            int flag = j == 0 ? 0 : 256; // primary / secondary
            if (sid % 2 == 1)
                flag |= 16; // reverse complement
            if (ctg) {
                const FastaContig &c = (*ctg->table)[(size_t)ctg->row_contig[i * k + (size_t)j]];
                append_aligned_row(buf, qname, flag, c.name, ref_len, query_seqs[g], sid, *aln, i * k + (size_t)j, mapq,
                                   c.start, qual, &tail);
                continue;
            }
            if (aln) {
                append_aligned_row(buf, qname, flag, ref_name, ref_len, query_seqs[g], sid, *aln, i * k + (size_t)j,
                                   mapq, 0, qual, &tail);
                continue;
            }
            buf += qname;
            buf += '\t';
            buf += std::to_string(flag);
            buf += '\t';
            buf += ref_name;
            buf += '\t';
            buf += std::to_string(sid / 2 + 1); // 1-based position
            buf += '\t';
            buf += mapq ? std::to_string(mapq[i * k + (size_t)j]) : std::string("60");
            buf += '\t';
            buf += cigar;
            buf += "\t*\t0\t0\t";
            buf += clean; // as read, also under flag 16: so is the quality line
            buf += '\t';
            buf += qual_col;
            buf += '\n';
        }
        // DRM_CONTIGS: a read without a row inside a contig is written unmapped; DRM_SAM_LOCI: a read without a locus
        if ((ctg || loci) && counts[i] < 1)
            buf += qname + "\t4\t*\t0\t0\t*\t*\t0\t0\t" + (clean.empty() ? std::string("*") : clean) + "\t" + qual_col +
                   "\n";
        if (buf.size() > (1u << 22)) {
            out << buf;
            buf.clear();
        }
    }
    out << buf;
}

// ----------------------------------------------------------------------- paired SAM (include/drm_hip.h)
static void sam_pair_fields(const drm_sam_mate in[2], bool proper, drm_sam_mate_fields out[2])
{
    using drm::Error;
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
    try {
        if (!in || !out)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        sam_pair_fields(in, proper != 0, out);
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_ARG;
    }
}

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
    try {
        if (!p || !start || !len || !reverse)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        if (glen < 0)
            throw drm::Error(DRM_ERR_ARG, "negative genome length");
        int64_t dlo = 0, dhi = 0;
        drm::check_rescue_params(p, dlo, dhi);
        const drm::RescueRegion r = drm::rescue_region(anchor_id, glen, p->ref_len, dlo, dhi);
        *start = r.start;
        *len = r.len;
        *reverse = r.reverse;
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_ARG;
    }
}

extern "C" int drm_mate_rescue_window(const drm_rescue_result *r, int32_t ref_len, int64_t glen, uint64_t *window_id)
{
    try {
        if (!r || !window_id)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        *window_id = rescue_window(*r, ref_len, glen);
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_ARG;
    }
}

extern "C" int drm_pair_rescue_choose(const drm_pair_result *pair, int32_t s1, int32_t s2, uint64_t anchor1,
                                      uint64_t anchor2, const drm_rescue_result *rA, const drm_rescue_result *rB,
                                      int32_t ref_len, int64_t glen, int32_t unpaired_penalty, int32_t min_score,
                                      drm_pair_result *out, uint64_t *rescued_id)
{
    try {
        if (!pair || !out || !rescued_id)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        drm_pair_result o{};
        uint64_t w = 0;
        pair_rescue_choose(*pair, s1, s2, anchor1, anchor2, rA, rB, ref_len, glen, unpaired_penalty, min_score, o, w);
        *out = o;
        *rescued_id = w;
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_ARG;
    }
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
    try {
        if (!mapq)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        *mapq = mapq_value_checked(s1, sub, n_sub, full, min_score);
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_ARG;
    }
}

extern "C" int drm_pair_mapq_rescued(const drm_mapq_params *mp, const drm_pair_result *pairs,
                                     const int32_t *rescue_score, const int32_t *full1, const int32_t *full2,
                                     int64_t npairs, int64_t row_step, drm_pair_mapq_result *inout)
{
    try {
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
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_ARG;
    }
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
    try {
        if (!hist_row || !out)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        if (nbins < 2 || nbins > (1 << 16) + 1)
            throw drm::Error(DRM_ERR_ARG, "nbins " + std::to_string(nbins) + " outside [2, 2^16 + 1]");
        if (min_samples < 1)
            throw drm::Error(DRM_ERR_ARG, "min_samples " + std::to_string(min_samples) + " must be >= 1");
        *out = tlen_estimate(hist_row, nbins, min_samples);
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_ARG;
    }
}

void drm::write_sam_pairs(const std::string &path, bool header, const std::string &ref_name, size_t ref_len,
                          const std::vector<std::string> &query_seqs, const std::vector<std::string> &query_ids,
                          size_t q0, size_t npairs, const uint64_t *ids, const int32_t *counts, const int32_t *proper,
                          const SamAlignments &aln, const int32_t *mapq, const SamContigs *ctg,
                          const std::vector<std::string> *quals, const SamXa *xa)
{
    if (quals && quals->empty())
        quals = nullptr;
    std::ofstream out(path, header ? std::ios::out : std::ios::app);
    if (!out.is_open())
        throw Error(DRM_ERR_IO, "Failed to open SAM file: " + path);
    if (header)
        sam_header(out, ref_name, ref_len, ctg);
    std::string buf;
    for (size_t p = 0; p < npairs; ++p) {
        drm_sam_mate in[2];
        drm_sam_mate_fields f[2];
        std::string cigar[2], clean[2];
        for (int m = 0; m < 2; ++m) {
            const size_t row = 2 * p + (size_t)m;
            const std::string &tagged = query_seqs[q0 + row];
            // the read is the query without format_fastq's tags, as in the DRM_SAM_CIGAR row
            const int pre = !tagged.empty() && tagged.front() == '<', post = tagged.size() > 1 && tagged.back() == '>';
            clean[m] = tagged.substr((size_t)pre, tagged.size() - (size_t)pre - (size_t)post);
            const drm_sw_alignment &a = aln.rec[row];
            in[m] = drm_sam_mate{0, 0, 0, 0};
            if (counts[row] < 1 || a.status == 1)
                continue;
            const uint64_t sid = ids[row];
            int64_t pos1 = 0;
            if (aln.region_start)
                sam_cigar(a, aln.ops + aln.ops_off[row], (int32_t)tagged.size(), pre, post, aln.region_start[row],
                          aln.region_len[row], (sid & 1u) != 0, pos1, cigar[m]);
            else
                sam_cigar(a, aln.ops + aln.ops_off[row], (int32_t)tagged.size(), pre, post, (int64_t)(sid / 2),
                          (int32_t)ref_len, (sid & 1u) != 0, pos1, cigar[m]);
            if (ctg) // DRM_CONTIGS: the contig's own coordinate
                pos1 -= (*ctg->table)[(size_t)ctg->row_contig[row]].start;
            in[m] = drm_sam_mate{1, (int32_t)(sid & 1u), pos1, a.ref_end - a.ref_begin};
        }
        // DRM_CONTIGS: RNAME is the contig of the line's own position (an unmapped mate takes its mate's), RNEXT "=" on
        // one contig; mates on two contigs are never a proper pair and have no template length
        const std::string *rname[2] = {&ref_name, &ref_name};
        bool split = false;
        if (ctg) {
            for (int m = 0; m < 2; ++m) {
                const int src = in[m].mapped ? m : 1 - m;
                if (in[src].mapped)
                    rname[m] = &(*ctg->table)[(size_t)ctg->row_contig[2 * p + (size_t)src]].name;
            }
            split = in[0].mapped && in[1].mapped && ctg->row_contig[2 * p] != ctg->row_contig[2 * p + 1];
        }
        sam_pair_fields(in, proper[p] != 0 && !split, f);
        if (split)
            f[0].tlen = f[1].tlen = 0;
        const size_t g = q0 + 2 * p;
        const std::string qname = (g < query_ids.size() && !query_ids[g].empty()) ? query_ids[g]
                                                                                  : "S1/" + std::to_string(g / 2 + 1) + "/0";
        for (int m = 0; m < 2; ++m) {
            buf += qname;
            buf += '\t';
            buf += std::to_string(f[m].flag);
            buf += '\t';
            buf += f[m].has_rname ? *rname[m] : std::string("*");
            buf += '\t';
            buf += std::to_string(f[m].pos);
            buf += '\t';
            buf += mapq ? std::to_string(in[m].mapped ? mapq[2 * p + (size_t)m] : 0) : std::string("60");
            buf += '\t';
            buf += in[m].mapped ? cigar[m] : std::string("*");
            buf += !f[m].has_rname ? "\t*\t" : split ? "\t" + *rname[1 - m] + "\t" : std::string("\t=\t");
            buf += std::to_string(f[m].pnext);
            buf += '\t';
            buf += std::to_string(f[m].tlen);
            buf += '\t';
            buf += clean[m].empty() ? std::string("*")
                                    : (in[m].mapped && in[m].reverse) ? drm::reverse_complement(clean[m]) : clean[m];
            const std::string *qual = quals ? &(*quals)[q0 + 2 * p + (size_t)m] : nullptr;
            buf += '\t';
            buf += !qual || qual->empty()           ? std::string("*")
                   : (in[m].mapped && in[m].reverse) ? std::string(qual->rbegin(), qual->rend())
                                                     : *qual;
            if (in[m].mapped) {
                buf += "\tAS:i:" + std::to_string(aln.rec[2 * p + (size_t)m].score);
                buf += "\tNM:i:" + std::to_string(aln.rec[2 * p + (size_t)m].nm);
                append_md_tag(buf, aln, 2 * p + (size_t)m, in[m].reverse != 0);
                if (xa) // DRM_SAM_LOCI: the mate's other loci
                    buf += xa_tag(*xa, 2 * p + (size_t)m, query_seqs[q0 + 2 * p + (size_t)m], ref_name, ref_len);
            }
            buf += '\n';
        }
        if (buf.size() > (1u << 22)) {
            out << buf;
            buf.clear();
        }
    }
    out << buf;
}

extern "C" int drm_extract_fasta_sequence(const char *path, uint8_t *out, int64_t *len)
{
    try {
        if (!path || !len)
            throw drm::Error(DRM_ERR_ARG, "null argument");
        const std::string g = drm::extract_fasta_sequence(path);
        if (out)
            std::memcpy(out, g.data(), std::min<size_t>(g.size(), (size_t)std::max<int64_t>(*len, 0)));
        *len = (int64_t)g.size();
        return DRM_OK;
    } catch (const drm::Error &e) {
        drm::set_last_error(e.what());
        return e.code;
    } catch (const std::exception &e) {
        drm::set_last_error(e.what());
        return DRM_ERR_IO;
    }
}
