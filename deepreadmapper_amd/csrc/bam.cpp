// deepreadmapper_amd/csrc/bam.cpp -- the BAM side of the SAM writer (include/drm_hip.h, "BAM output"): the one encoder
// of an alignment record (bam_encode_line, fed a SamLine by the writers of sam.cpp and by drm_bam_record, which parses
// its text into one), the BAM header, the fixed numbers of BGZF, and the run's sink (BamFile), which hands the encoded
// bytes to the device's compressor (drm_bgzf_compress, bgzf.hip) in whole BGZF blocks.
#include <chrono>
#include <cstdio>
#include <cstring>

#include <climits>

#include "drm_internal.h"

using namespace drm;

namespace {

void put_u8(std::string &o, uint32_t v) { o.push_back((char)(v & 255u)); }
void put_u16(std::string &o, uint32_t v)
{
    put_u8(o, v);
    put_u8(o, v >> 8);
}
void put_u32(std::string &o, uint32_t v)
{
    put_u16(o, v);
    put_u16(o, v >> 16);
}

// SAMv1 sec. 5.3, with arithmetic shifts: beg = -1 gives 4680
int reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14)
        return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17)
        return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20)
        return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23)
        return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26)
        return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

int64_t ref_id(std::string_view name, const SamRefIds &refs, const char *column)
{
    if (name == "*")
        return -1;
    const auto it = refs.find(name);
    if (it == refs.end())
        throw Error(DRM_ERR_ARG, std::string(column) + " " + std::string(name) + " is not among the reference names");
    return it->second;
}

// all of s as a decimal number with an optional sign; false when it is anything else
bool parse_int(std::string_view s, int64_t &v)
{
    size_t i = 0;
    const bool neg = !s.empty() && s[0] == '-';
    if (!s.empty() && (s[0] == '-' || s[0] == '+'))
        i = 1;
    if (i == s.size() || s.size() - i > 18)
        return false;
    v = 0;
    for (; i < s.size(); ++i) {
        if (s[i] < '0' || s[i] > '9')
            return false;
        v = v * 10 + (s[i] - '0');
    }
    if (neg)
        v = -v;
    return true;
}

// the CIGAR's words, len << 4 | op over MIDNSHP=X, and the reference bases it covers
void parse_cigar(std::string_view c, std::vector<uint32_t> &ops, int64_t &ref_len)
{
    static const std::string_view kOps = "MIDNSHP=X";
    ops.clear();
    ref_len = 0;
    if (c == "*")
        return;
    size_t i = 0;
    while (i < c.size()) {
        uint64_t n = 0;
        const size_t from = i;
        while (i < c.size() && c[i] >= '0' && c[i] <= '9' && n < ((uint64_t)1 << 28))
            n = n * 10 + (uint64_t)(c[i++] - '0');
        const size_t op = i < c.size() ? kOps.find(c[i]) : std::string_view::npos;
        if (i == from || op == std::string_view::npos || n >= ((uint64_t)1 << 28))
            throw Error(DRM_ERR_ARG, "CIGAR " + std::string(c) + " does not parse");
        ++i;
        ops.push_back((uint32_t)(n << 4) | (uint32_t)op);
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8)
            ref_len += (int64_t)n;
    }
    if (ops.empty())
        throw Error(DRM_ERR_ARG, "an empty CIGAR");
}

uint32_t base_code(char c)
{
    static const std::string_view kBases = "=ACMGRSVTWYHKDBN";
    const size_t at = c == '\0' ? std::string_view::npos : kBases.find(c);
    return at == std::string_view::npos ? 15u : (uint32_t)at;
}

char complement(char c)
{
    switch (c) {
    case 'A': return 'T';
    case 'T': return 'A';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'N': return 'N';
    default: return '\0'; // what the text writer prints for such a letter
    }
}

// "\tXX:T:value" after "\tXX:T:value": i as the smallest integer type that holds the value, Z, A
void encode_tags(std::string_view tags, std::string &o)
{
    size_t i = 0;
    while (i < tags.size()) {
        if (tags[i] != '\t')
            throw Error(DRM_ERR_INTERNAL, "a tag does not start a column");
        size_t end = tags.find('\t', i + 1);
        end = end == std::string_view::npos ? tags.size() : end;
        const std::string_view t = tags.substr(i + 1, end - i - 1);
        i = end;
        if (t.size() < 5 || t[2] != ':' || t[4] != ':')
            throw Error(DRM_ERR_ARG, "tag " + std::string(t) + " is not XX:T:value");
        const std::string_view value = t.substr(5);
        o.append(t.substr(0, 2));
        if (t[3] == 'i') {
            int64_t v = 0;
            if (!parse_int(value, v) || v < INT32_MIN || v > (int64_t)UINT32_MAX)
                throw Error(DRM_ERR_ARG, "tag " + std::string(t) + " holds no 32-bit number");
            if (v >= 0) { // samtools' rule: the smallest type
                o.push_back(v <= 255 ? 'C' : v <= 65535 ? 'S' : 'I');
                v <= 255 ? put_u8(o, (uint32_t)v) : v <= 65535 ? put_u16(o, (uint32_t)v) : put_u32(o, (uint32_t)v);
            } else {
                o.push_back(v >= -128 ? 'c' : v >= -32768 ? 's' : 'i');
                v >= -128 ? put_u8(o, (uint32_t)v) : v >= -32768 ? put_u16(o, (uint32_t)v) : put_u32(o, (uint32_t)v);
            }
        } else if (t[3] == 'Z') {
            o.push_back('Z');
            o.append(value).push_back('\0');
        } else if (t[3] == 'A') {
            if (value.size() != 1)
                throw Error(DRM_ERR_ARG, "tag " + std::string(t) + ": an A value is one character");
            o.push_back('A');
            o.push_back(value[0]);
        } else {
            throw Error(DRM_ERR_UNSUPPORTED, "tag " + std::string(t) + ": only the types i, Z and A are encoded");
        }
    }
}

} // namespace

void drm::bam_encode_line(const SamLine &l, const SamRefIds &refs, std::string &o)
{
    if (l.qname.size() > 254)
        throw Error(DRM_ERR_UNSUPPORTED, "a QNAME of " + std::to_string(l.qname.size()) + " bytes: BAM holds 254");
    if (l.flag < 0 || l.flag > 65535 || l.mapq < 0 || l.mapq > 255)
        throw Error(DRM_ERR_ARG, "FLAG outside [0, 65535] or MAPQ outside [0, 255]");
    if (l.pos < 0 || l.pos > INT32_MAX || l.pnext < 0 || l.pnext > INT32_MAX || l.tlen < INT32_MIN || l.tlen > INT32_MAX)
        throw Error(DRM_ERR_ARG, "POS, PNEXT or TLEN outside 32 bits");
    if (!l.qual.empty() && l.qual.size() != l.read.size())
        throw Error(DRM_ERR_ARG, "QUAL of " + std::to_string(l.qual.size()) + " characters for a SEQ of " +
                                     std::to_string(l.read.size()));
    const int64_t tid = ref_id(l.rname, refs, "RNAME");
    const int64_t next = l.rnext == "=" ? tid : ref_id(l.rnext, refs, "RNEXT");
    std::vector<uint32_t> ops;
    int64_t ref_len = 0;
    parse_cigar(l.cigar, ops, ref_len);
    if (ops.size() > 65535)
        throw Error(DRM_ERR_UNSUPPORTED, "a CIGAR of more than 65,535 operations");
    const int64_t pos = l.pos - 1;
    const size_t at = o.size();
    put_u32(o, 0); // block_size, known at the end
    put_u32(o, (uint32_t)(int32_t)tid);
    put_u32(o, (uint32_t)(int32_t)pos);
    put_u8(o, (uint32_t)l.qname.size() + 1);
    put_u8(o, (uint32_t)l.mapq);
    put_u16(o, (uint32_t)reg2bin(pos, pos + std::max<int64_t>(1, ref_len)));
    put_u16(o, (uint32_t)ops.size());
    put_u16(o, (uint32_t)l.flag);
    put_u32(o, (uint32_t)l.read.size());
    put_u32(o, (uint32_t)(int32_t)next);
    put_u32(o, (uint32_t)(int32_t)(l.pnext - 1));
    put_u32(o, (uint32_t)(int32_t)l.tlen);
    o.append(l.qname).push_back('\0');
    for (uint32_t w : ops)
        put_u32(o, w);
    const size_t n = l.read.size();
    auto base = [&](size_t i) { return l.reversed ? complement(l.read[n - 1 - i]) : l.read[i]; };
    for (size_t i = 0; i < n; i += 2)
        put_u8(o, base_code(base(i)) << 4 | (i + 1 < n ? base_code(base(i + 1)) : 0u));
    for (size_t i = 0; i < n; ++i)
        put_u8(o, l.qual.empty() ? 0xFFu : (uint32_t)(unsigned char)l.qual[l.reversed ? n - 1 - i : i] - 33u);
    encode_tags(l.tags, o);
    const uint32_t size = (uint32_t)(o.size() - at - 4);
    for (int b = 0; b < 4; ++b)
        o[at + (size_t)b] = (char)((size >> (8 * b)) & 255u);
}

void drm::bam_encode_header(std::string_view text, std::string &o)
{
    o.append("BAM\1", 4);
    put_u32(o, (uint32_t)text.size());
    o.append(text);
    const size_t n_ref_at = o.size();
    put_u32(o, 0);
    uint32_t n_ref = 0;
    for (size_t from = 0; from < text.size();) {
        size_t end = text.find('\n', from);
        end = end == std::string_view::npos ? text.size() : end;
        const std::string_view line = text.substr(from, end - from);
        from = end + 1;
        if (line.substr(0, 4) != "@SQ\t")
            continue;
        std::string_view name;
        int64_t len = -1;
        for (size_t f = 4; f <= line.size();) {
            size_t fe = line.find('\t', f);
            fe = fe == std::string_view::npos ? line.size() : fe;
            const std::string_view field = line.substr(f, fe - f);
            if (field.substr(0, 3) == "SN:")
                name = field.substr(3);
            else if (field.substr(0, 3) == "LN:" && (!parse_int(field.substr(3), len) || len < 0 || len > INT32_MAX))
                throw Error(DRM_ERR_ARG, "@SQ line with LN that is no 31-bit number: " + std::string(line));
            f = fe + 1;
        }
        if (name.empty() || len < 0)
            throw Error(DRM_ERR_ARG, "@SQ line without SN or LN: " + std::string(line));
        put_u32(o, (uint32_t)name.size() + 1);
        o.append(name).push_back('\0');
        put_u32(o, (uint32_t)len);
        ++n_ref;
    }
    for (int b = 0; b < 4; ++b)
        o[n_ref_at + (size_t)b] = (char)((n_ref >> (8 * b)) & 255u);
}

// ----------------------------------------------------------------------------------------- C ABI (host only)
static void give(const std::string &o, uint8_t *out, size_t cap, size_t *bytes)
{
    *bytes = o.size();
    if (o.size() > cap)
        throw Error(DRM_ERR_ARG, "cap " + std::to_string(cap) + " is too small for " + std::to_string(o.size()) + " bytes");
    if (!o.empty())
        std::memcpy(out, o.data(), o.size());
}

extern "C" int drm_bam_header(const char *sam_header_text, size_t len, uint8_t *out, size_t cap, size_t *bytes)
{
    return drm::guarded([&] {
        if ((!sam_header_text && len > 0) || !out || !bytes)
            throw Error(DRM_ERR_ARG, "null argument");
        std::string o;
        bam_encode_header(std::string_view(sam_header_text ? sam_header_text : "", len), o);
        give(o, out, cap, bytes);
    });
}

extern "C" int drm_bam_record(const char *line, size_t len, const char *const *ref_names, int32_t n_ref, uint8_t *out,
                              size_t cap, size_t *bytes)
{
    return drm::guarded([&] {
        if (!line || !out || !bytes || n_ref < 0 || (n_ref > 0 && !ref_names))
            throw Error(DRM_ERR_ARG, "null argument or negative n_ref");
        std::string_view text(line, len);
        if (!text.empty() && text.back() == '\n')
            text.remove_suffix(1);
        SamRefIds refs;
        for (int32_t i = 0; i < n_ref; ++i) {
            if (!ref_names[i])
                throw Error(DRM_ERR_ARG, "null reference name");
            refs.emplace(ref_names[i], i); // a repeated name keeps its first index
        }
        std::string_view col[11];
        size_t from = 0; // behind the loop: the tab in front of the first tag, or the end
        int c = 0;
        for (; c < 11; ++c) {
            const size_t tab = text.find('\t', from), end = tab == std::string_view::npos ? text.size() : tab;
            col[c] = text.substr(from, end - from);
            from = end;
            if (c < 10) {
                if (tab == std::string_view::npos)
                    break;
                ++from;
            }
        }
        if (c < 11)
            throw Error(DRM_ERR_ARG, "a SAM line has eleven columns, this one " + std::to_string(c + 1));
        int64_t num[5];
        const int which[5] = {1, 3, 4, 7, 8};
        for (int i = 0; i < 5; ++i)
            if (!parse_int(col[which[i]], num[i]))
                throw Error(DRM_ERR_ARG, "column " + std::to_string(which[i] + 1) + " is not a number: " +
                                             std::string(col[which[i]]));
        if (col[0].empty() || col[9].empty() || col[10].empty())
            throw Error(DRM_ERR_ARG, "an empty QNAME, SEQ or QUAL");
        if (col[9] == "*" && col[10] != "*")
            throw Error(DRM_ERR_ARG, "QUAL without SEQ");
        SamLine l;
        l.qname = col[0];
        if (num[0] < 0 || num[0] > 65535 || num[2] < 0 || num[2] > 255)
            throw Error(DRM_ERR_ARG, "FLAG outside [0, 65535] or MAPQ outside [0, 255]");
        l.flag = (int)num[0];
        l.rname = col[2];
        l.pos = num[1];
        l.mapq = (int)num[2];
        l.cigar = col[5];
        l.rnext = col[6];
        l.pnext = num[3];
        l.tlen = num[4];
        l.read = col[9] == "*" ? std::string_view() : col[9];
        l.qual = col[10] == "*" ? std::string_view() : col[10];
        l.tags = std::string(text.substr(from));
        std::string o;
        bam_encode_line(l, refs, o);
        give(o, out, cap, bytes);
    });
}

extern "C" int drm_bgzf_block(void) { return kBgzfBlock; }

extern "C" int drm_bgzf_bound(int64_t n, size_t *bytes)
{
    return drm::guarded([&] {
        if (!bytes)
            throw Error(DRM_ERR_ARG, "null argument");
        if (n < 0)
            throw Error(DRM_ERR_ARG, "n must be >= 0");
        *bytes = (size_t)n + 31 * (size_t)((n + kBgzfBlock - 1) / kBgzfBlock);
    });
}

static const uint8_t kBgzfEof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

extern "C" int drm_bgzf_eof(uint8_t out[28])
{
    return drm::guarded([&] {
        if (!out)
            throw Error(DRM_ERR_ARG, "null argument");
        std::memcpy(out, kBgzfEof, sizeof kBgzfEof);
    });
}

// ----------------------------------------------------------------------------------------------- the sink
void BamFile::encode(const SamLine &l, const SamRefIds &refs, std::string &to) { bam_encode_line(l, refs, to); }

void BamFile::begin(const std::string &path, std::string_view header_text)
{
    if (file)
        throw Error(DRM_ERR_INTERNAL, "the BAM file is open already");
    file = std::fopen(path.c_str(), "wb");
    if (!file)
        throw Error(DRM_ERR_IO, "Failed to open BAM file: " + path);
    file_path = path;
    buf.clear();
    bam_encode_header(header_text, buf);
}

void BamFile::flush(bool all)
{
    if (!file)
        throw Error(DRM_ERR_INTERNAL, "the BAM file is not open");
    // whole BGZF blocks only, so that the members do not depend on where the stream was cut; about 4 MiB at a time
    if (!all && buf.size() <= (1u << 22))
        return;
    const size_t take = all ? buf.size() : buf.size() / kBgzfBlock * kBgzfBlock;
    if (take == 0)
        return;
    size_t bound = 0, got = 0;
    if (drm_bgzf_bound((int64_t)take, &bound) != DRM_OK)
        throw Error(DRM_ERR_INTERNAL, drm_last_error());
    packed.resize(bound);
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = drm_bgzf_compress(reinterpret_cast<const uint8_t *>(buf.data()), (int64_t)take, device, packed.data(),
                                     packed.size(), &got);
    if (rc != DRM_OK)
        throw Error(rc, drm_last_error());
    compress_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    bytes_in += take;
    bytes_out += got;
    if (std::fwrite(packed.data(), 1, got, static_cast<std::FILE *>(file)) != got)
        throw Error(DRM_ERR_IO, "Failed to write BAM file: " + file_path);
    buf.erase(0, take);
}

void BamFile::finish()
{
    flush(true);
    std::FILE *f = static_cast<std::FILE *>(file);
    file = nullptr;
    const bool ok = std::fwrite(kBgzfEof, 1, sizeof kBgzfEof, f) == sizeof kBgzfEof;
    bytes_out += sizeof kBgzfEof;
    if (std::fclose(f) != 0 || !ok)
        throw Error(DRM_ERR_IO, "Failed to write BAM file: " + file_path);
}

BamFile::~BamFile()
{
    if (file)
        std::fclose(static_cast<std::FILE *>(file));
}
