"""BGZF and BAM restated from the specifications alone (RFC 1952 for the gzip member, SAMv1 sec. 4.1 for BGZF, sec. 4.2
for the alignment record, sec. 5.3 for the bin), with Python's zlib as the one inflater and CRC: a reader that takes a
BGZF file apart member by member and checks everything it passes, a decoder from BAM bytes to SAM text, and an encoder of
one SAM line and of a header that owes nothing to csrc/bam.cpp. A helper, not a test module."""
import struct
import zlib

BLOCK = 65280
HEAD = bytes.fromhex("1f8b08040000000000ff0600424302 00".replace(" ", ""))
EOF = HEAD + bytes.fromhex("1b0003000000000000000000")
BASES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"


class BgzfError(ValueError):
    pass


def member(payload_of, raw):
    """A BGZF member around raw's DEFLATE payload, for building reader inputs: payload_of(raw) -> bytes."""
    payload = payload_of(raw)
    size = 18 + len(payload) + 8
    return HEAD + struct.pack("<H", size - 1) + payload + struct.pack("<II", zlib.crc32(raw), len(raw))


def zlib_member(raw, level=6):
    def payload(b):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        return c.compress(b) + c.flush()
    return member(payload, raw)


def read_bgzf(data, eof=True):
    """(the inflated bytes, [BTYPE of every member's first DEFLATE block], [every member's inflated length]). Every
    header byte, BSIZE (it must land on the next member, and the last on the end of the data), the payload (inflated
    alone, with no window from the member before, and ending exactly where the trailer starts), CRC-32 and ISIZE are
    checked; with `eof` the data must end with the empty EOF member. BgzfError names the first fault."""
    data = bytes(data)
    out, btypes, sizes = [], [], []
    at = 0
    while at < len(data):
        if len(data) - at < 18 + 2 + 8:
            raise BgzfError(f"{len(data) - at} bytes at {at} are no member")
        if data[at:at + 16] != HEAD:
            raise BgzfError(f"header bytes at {at}: {data[at:at + 16].hex()}")
        bsize = struct.unpack_from("<H", data, at + 16)[0] + 1
        if bsize < 18 + 2 + 8 or at + bsize > len(data):
            raise BgzfError(f"BSIZE {bsize} at {at} with {len(data) - at} bytes left")
        payload = data[at + 18:at + bsize - 8]
        d = zlib.decompressobj(-15)
        try:
            raw = d.decompress(payload)
        except zlib.error as e:
            raise BgzfError(f"member at {at}: {e}")
        if not d.eof or d.unused_data:
            raise BgzfError(f"member at {at}: the DEFLATE stream does not end at the trailer "
                            f"(eof {d.eof}, {len(d.unused_data)} bytes left)")
        crc, isize = struct.unpack_from("<II", data, at + bsize - 8)
        if crc != zlib.crc32(raw):
            raise BgzfError(f"member at {at}: CRC {crc:08x}, the bytes have {zlib.crc32(raw):08x}")
        if isize != len(raw):
            raise BgzfError(f"member at {at}: ISIZE {isize} for {len(raw)} bytes")
        if len(raw) > BLOCK:
            raise BgzfError(f"member at {at} holds {len(raw)} bytes")
        out.append(raw)
        btypes.append((payload[0] >> 1) & 3)
        sizes.append(len(raw))
        at += bsize
    if eof and (data[-28:] != EOF or not sizes or sizes[-1] != 0):
        raise BgzfError("no EOF member at the end")
    return b"".join(out), btypes, sizes


def reg2bin(beg, end):
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return first + (beg >> shift)
    return 0


def _int_tag(v):
    if v >= 0:
        return (b"C", "<B") if v <= 0xFF else (b"S", "<H") if v <= 0xFFFF else (b"I", "<I")
    return (b"c", "<b") if v >= -0x80 else (b"s", "<h") if v >= -0x8000 else (b"i", "<i")


def encode_record(line, ref_names):
    """The BAM alignment record of one SAM line, block_size first (SAMv1 sec. 4.2)."""
    f = line.rstrip("\n").split("\t")
    assert len(f) >= 11, line
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    names = list(ref_names)
    tid = -1 if rname == "*" else names.index(rname)
    ntid = -1 if rnext == "*" else tid if rnext == "=" else names.index(rnext)
    ops, ref_len, num = [], 0, ""
    if cigar != "*":
        for ch in cigar:
            if ch.isdigit():
                num += ch
            else:
                ops.append(int(num) << 4 | CIGAR_OPS.index(ch))
                ref_len += int(num) if ch in "MDN=X" else 0
                num = ""
    p0 = int(pos) - 1
    l_seq = 0 if seq == "*" else len(seq)
    name = qname.encode() + b"\0"
    body = struct.pack("<iiBBHHHIiii", tid, p0, len(name), int(mapq), reg2bin(p0, p0 + max(1, ref_len)) & 0xFFFF,
                       len(ops), int(flag), l_seq, ntid, int(pnext) - 1, int(tlen))
    body += name + b"".join(struct.pack("<I", w) for w in ops)
    nib = [BASES.index(c) if c in BASES else 15 for c in (seq if l_seq else "")]
    nib += [0] * (len(nib) & 1)
    body += bytes(nib[i] << 4 | nib[i + 1] for i in range(0, len(nib), 2))
    body += bytes([0xFF] * l_seq) if qual == "*" else bytes(ord(c) - 33 for c in qual)
    for t in f[11:]:
        tag, typ, val = t[:2], t[3], t[5:]
        if typ == "i":
            code, fmt = _int_tag(int(val))
            body += tag.encode() + code + struct.pack(fmt, int(val))
        elif typ == "Z":
            body += tag.encode() + b"Z" + val.encode() + b"\0"
        elif typ == "A":
            body += tag.encode() + b"A" + val.encode()
        else:
            raise ValueError(t)
    return struct.pack("<I", len(body)) + body


def encode_header(text):
    """The uncompressed BAM header of a SAM header text: one reference per @SQ line, in order."""
    t = text.encode()
    refs = []
    for line in text.split("\n"):
        if line.startswith("@SQ\t"):
            kv = dict(x.split(":", 1) for x in line.split("\t")[1:])
            refs.append((kv["SN"], int(kv["LN"])))
    out = b"BAM\1" + struct.pack("<I", len(t)) + t + struct.pack("<I", len(refs))
    for name, ln in refs:
        out += struct.pack("<I", len(name) + 1) + name.encode() + b"\0" + struct.pack("<I", ln)
    return out


_TAG_INTS = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


def decode_record(rec, names):
    """One SAM line (no newline) from one alignment record without its block_size; every integer tag prints as i."""
    tid, p0, l_name, mapq, bin_, n_ops, flag, l_seq, ntid, np0, tlen = struct.unpack_from("<iiBBHHHIiii", rec, 0)
    at = 32
    assert rec[at + l_name - 1] == 0, "QNAME without NUL"
    qname = rec[at:at + l_name - 1].decode()
    at += l_name
    ops = struct.unpack_from(f"<{n_ops}I", rec, at)
    at += 4 * n_ops
    cigar = "".join(f"{w >> 4}{CIGAR_OPS[w & 15]}" for w in ops) or "*"
    ref_len = sum(w >> 4 for w in ops if CIGAR_OPS[w & 15] in "MDN=X")
    assert bin_ == reg2bin(p0, p0 + max(1, ref_len)) & 0xFFFF, ("bin", bin_, p0, ref_len)
    packed = rec[at:at + (l_seq + 1) // 2]
    at += (l_seq + 1) // 2
    seq = "".join(BASES[packed[i >> 1] >> 4 if i % 2 == 0 else packed[i >> 1] & 15] for i in range(l_seq)) or "*"
    assert l_seq % 2 == 0 or packed[-1] & 15 == 0, "the spare nibble is not 0"
    q = rec[at:at + l_seq]
    at += l_seq
    qual = "*" if l_seq == 0 or all(x == 0xFF for x in q) else "".join(chr(x + 33) for x in q)
    tags = []
    while at < len(rec):
        tag, typ = rec[at:at + 2].decode(), chr(rec[at + 2])
        at += 3
        if typ in _TAG_INTS:
            fmt = _TAG_INTS[typ]
            tags.append(f"{tag}:i:{struct.unpack_from(fmt, rec, at)[0]}")
            at += struct.calcsize(fmt)
        elif typ == "Z":
            end = rec.index(b"\0", at)
            tags.append(f"{tag}:Z:{rec[at:end].decode()}")
            at = end + 1
        elif typ == "A":
            tags.append(f"{tag}:A:{chr(rec[at])}")
            at += 1
        else:
            raise ValueError(f"tag type {typ}")
    assert at == len(rec), "the tags run past the record"
    rname = "*" if tid < 0 else names[tid]
    rnext = "*" if ntid < 0 else "=" if ntid == tid else names[ntid]
    return "\t".join([qname, str(flag), rname, str(p0 + 1), str(mapq), cigar, rnext, str(np0 + 1), str(tlen), seq, qual]
                     + tags)


def decode_bam(raw):
    """The SAM text lines (header lines, then one per record) of uncompressed BAM bytes."""
    assert raw[:4] == b"BAM\1", raw[:4]
    l_text = struct.unpack_from("<I", raw, 4)[0]
    text = raw[8:8 + l_text].decode()
    at = 8 + l_text
    n_ref = struct.unpack_from("<I", raw, at)[0]
    at += 4
    names, lens = [], []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<I", raw, at)[0]
        assert raw[at + 4 + l_name - 1] == 0
        names.append(raw[at + 4:at + 4 + l_name - 1].decode())
        lens.append(struct.unpack_from("<I", raw, at + 4 + l_name)[0])
        at += 8 + l_name
    assert raw[:at] == encode_header(text), "the references are not the text's @SQ lines"
    lines = text.split("\n")
    assert lines[-1] == "", "the header text does not end a line"
    lines = lines[:-1]
    while at < len(raw):
        size = struct.unpack_from("<I", raw, at)[0]
        assert size >= 32 and at + 4 + size <= len(raw), ("block_size", size, at)
        lines.append(decode_record(raw[at + 4:at + 4 + size], names))
        at += 4 + size
    return lines
