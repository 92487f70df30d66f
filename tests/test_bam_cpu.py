"""CPU tests of the BAM side that needs no device: the BGZF reader of tests/bam_ref.py is a yardstick that accepts zlib's
own members and rejects a flipped CRC byte, a wrong BSIZE, a wrong ISIZE and a missing EOF member; drm_bam_record equals
the independent Python encoder byte for byte and decodes back to its line, on every kind of line the writers produce and
on the edges of every field; each malformed line gives its error; drm_bam_header equals the Python restatement; the fixed
numbers of BGZF; bin/pipeline refuses a bad DRM_SAM_FORMAT, and the switch without its companions, before the index is
loaded."""
import os
import random
import struct
import subprocess
import zlib

import pytest

import bam_ref as B
from conftest import ROOT

NAMES = ["chr1", "chr2", "chrM"]
SEQ = "ACGTTGCANACGT"
MAPPED = "r1\t0\tchr1\t100\t37\t3S10M\t*\t0\t0\t" + SEQ + "\tIIIIIHHHHGGF#\tAS:i:10\tNM:i:0\tMD:Z:10\tXA:Z:chr2,-57,13M,1;"


def _both(line, names=NAMES):
    """The record of `line`: equal to the Python encoder's, and decoding back to the line (a base outside the alphabet
    comes back as N, which is what code 15 means)."""
    from deepreadmapper_amd import bam_record
    got = bam_record(line, names)
    assert got == B.encode_record(line, names), line
    size = struct.unpack_from("<I", got, 0)[0]
    assert size == len(got) - 4
    f = line.split("\t")
    f[9] = "".join(c if c in B.BASES or c == "*" else "N" for c in f[9])
    assert B.decode_record(got[4:], names) == "\t".join(f)
    return got


# ---------------------------------------------------------------------------------------------------- the reader
def _file():
    rng = random.Random(5)
    a = bytes(rng.randrange(4) for _ in range(70000))
    raws = [a[:B.BLOCK], a[B.BLOCK:], b"x" * 1000]
    return b"".join(raws), b"".join(B.zlib_member(r) for r in raws) + B.EOF


def test_reader_accepts_zlibs_members_and_returns_their_bytes():
    raw, data = _file()
    got, btypes, sizes = B.read_bgzf(data)
    assert got == raw and sizes == [B.BLOCK, 70000 - B.BLOCK, 1000, 0]
    assert btypes == [2, 2, 1, 1]  # dynamic where it pays, fixed for the run and for the EOF member
    stored = B.member(lambda b: b"\x01" + struct.pack("<HH", len(b), len(b) ^ 0xFFFF) + b, b"abc")
    assert B.read_bgzf(stored + B.EOF) == (b"abc", [0, 1], [3, 0])
    assert B.read_bgzf(B.EOF) == (b"", [1], [0])


def test_reader_rejects_every_fault():
    raw, data = _file()
    first = struct.unpack_from("<H", data, 16)[0] + 1

    def bad(change):
        d = bytearray(data)
        change(d)
        with pytest.raises(B.BgzfError):
            B.read_bgzf(bytes(d))

    bad(lambda d: d.__setitem__(first - 8, d[first - 8] ^ 1))          # a CRC byte of the first member
    bad(lambda d: d.__setitem__(slice(16, 18), struct.pack("<H", first)))      # BSIZE one too large
    bad(lambda d: d.__setitem__(slice(16, 18), struct.pack("<H", first - 2)))  # BSIZE one too small
    bad(lambda d: d.__setitem__(first - 4, d[first - 4] ^ 1))          # ISIZE
    bad(lambda d: d.__setitem__(3, 0))                                 # FLG without FEXTRA
    bad(lambda d: d.__setitem__(12, ord("X")))                         # the subfield's name
    bad(lambda d: d.__delitem__(slice(len(d) - 28, len(d))))           # no EOF member
    bad(lambda d: d.__delitem__(slice(len(d) - 1, len(d))))            # a cut file
    bad(lambda d: d.extend(b"\0"))                                     # a byte behind the EOF member
    assert B.read_bgzf(data[:-28], eof=False)[0] == raw
    # a member whose payload leans on the member before cannot be inflated alone
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    one = c.compress(raw[:1000]) + c.flush(zlib.Z_FULL_FLUSH)
    c2 = zlib.compressobj(6, zlib.DEFLATED, -15, zdict=raw[:1000])
    two = B.member(lambda b: c2.compress(b) + c2.flush(), raw[:1000])
    with pytest.raises(B.BgzfError):
        B.read_bgzf(B.member(lambda b: one + b"\x03\x00", raw[:1000]) + two + B.EOF)


# --------------------------------------------------------------------------------------------------- the records
LINES = {
    "mapped_forward": MAPPED,
    "reverse": "r2\t16\tchr2\t5\t60\t13M\t*\t0\t0\t" + SEQ + "\t" + "I" * 13 + "\tAS:i:13\tNM:i:0",
    "unmapped": "r3\t4\t*\t0\t0\t*\t*\t0\t0\t" + SEQ + "\t" + "#" * 13,
    "unmapped_mate_at_its_mates_position": "r4\t69\tchr1\t250\t0\t*\t=\t250\t0\t" + SEQ + "\t" + "5" * 13,
    "rnext_equal_negative_tlen": "r5\t147\tchr1\t400\t60\t13M\t=\t200\t-213\t" + SEQ + "\t" + "I" * 13 + "\tAS:i:13\tNM:i:0",
    "rnext_named": "r6\t65\tchr1\t400\t60\t13M\tchrM\t7\t0\t" + SEQ + "\t" + "I" * 13,
    "odd_seq": "r7\t0\tchr1\t1\t1\t3M\t*\t0\t0\tACG\t!~J",
    "seq_star": "r8\t0\tchr1\t1\t1\t3M\t*\t0\t0\t*\t*",
    "qual_star": "r9\t0\tchr1\t1\t1\t4M\t*\t0\t0\tACGT\t*",
    "base_outside_the_alphabet": "r10\t0\tchr1\t1\t1\t6M\t*\t0\t0\tACXT=N\tIIIIII",
    "int_tags": "r11\t0\tchr1\t1\t1\t1M\t*\t0\t0\tA\tI\t" + "\t".join(
        f"X{chr(ord('a') + i)}:i:{v}" for i, v in enumerate((0, 255, 256, 65535, 65536, -1, -128, -129, -32768, -32769,
                                                              2 ** 32 - 1, -2 ** 31))),
    "char_tag": "r12\t0\tchr1\t1\t1\t1M\t*\t0\t0\tA\tI\tXT:A:U\tRG:Z:",
    "qname_254": "q" * 254 + "\t0\tchr1\t1\t1\t1M\t*\t0\t0\tA\tI",
    "pos_beyond_2_29": "r13\t0\tchr2\t600000000\t9\t100M\t*\t0\t0\tA\tI",
    "every_operator": "r14\t0\tchr1\t70000\t9\t2H3S4M1I2D5N1P3=2X1S\t*\t0\t0\t" + "ACGTACGTACGTAC" + "\t" + "F" * 14,
    "span_over_a_bin_edge": "r15\t0\tchr1\t16380\t9\t10M\t*\t0\t0\tACGTACGTAC\tFFFFFFFFFF",
}


@pytest.mark.parametrize("case", sorted(LINES))
def test_record_equals_the_python_encoder_and_decodes_back(case):
    _both(LINES[case])


def test_fields_of_the_edge_cases():
    f = "<iiBBHHHIiii"
    u = struct.unpack_from(f, _both(LINES["unmapped"]), 4)
    assert u[0] == -1 and u[1] == -1 and u[4] == 4680 and u[5] == 0 and u[8] == -1 and u[9] == -1
    m = struct.unpack_from(f, _both(LINES["unmapped_mate_at_its_mates_position"]), 4)
    assert m[0] == 0 and m[1] == 249 and m[4] == B.reg2bin(249, 250) and m[8] == 0 and m[9] == 249
    n = struct.unpack_from(f, _both(LINES["rnext_named"]), 4)
    assert n[8] == 2 and n[9] == 6
    t = struct.unpack_from(f, _both(LINES["rnext_equal_negative_tlen"]), 4)
    assert t[8] == t[0] == 0 and t[10] == -213
    top = struct.unpack_from(f, _both(LINES["pos_beyond_2_29"]), 4)
    assert top[1] == 599999999 and top[4] == (4681 + (599999999 >> 14)) & 0xFFFF
    edge = struct.unpack_from(f, _both(LINES["span_over_a_bin_edge"]), 4)
    assert edge[4] == 585 + 0  # 16379 .. 16388 crosses 2^14: the level above
    rec = _both(LINES["base_outside_the_alphabet"])
    assert rec[4 + 32 + 4 + 4:4 + 32 + 4 + 4 + 3] == bytes([0x12, 0xF8, 0x0F])
    q = _both(LINES["qual_star"])
    assert q.endswith(bytes([0x12, 0x48]) + b"\xff" * 4)
    s = struct.unpack_from(f, _both(LINES["seq_star"]), 4)
    assert s[7] == 0
    body = _both(LINES["int_tags"])  # the types, in order
    at = 4 + 32 + 4 + 4 + 1 + 1
    types = []
    for width in (1, 1, 2, 2, 4, 1, 1, 2, 2, 4, 4, 4):
        types.append(chr(body[at + 2]))
        at += 3 + width
    assert at == len(body) and "".join(types) == "CCSSIccssiIi"


def test_malformed_lines_give_their_errors():
    from deepreadmapper_amd import DrmError, bam_record
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED
    ok = "r\t0\tchr1\t1\t1\t4M\t*\t0\t0\tACGT\tIIII"
    assert bam_record(ok, NAMES) == B.encode_record(ok, NAMES)
    assert bam_record(ok + "\n", NAMES) == B.encode_record(ok, NAMES)

    def field(i, v):
        f = ok.split("\t")
        f[i] = v
        return "\t".join(f)
    cases = [("\t".join(ok.split("\t")[:10]), DRM_ERR_ARG),      # ten columns
             ("", DRM_ERR_ARG),
             (field(1, "x"), DRM_ERR_ARG), (field(1, ""), DRM_ERR_ARG), (field(1, "65536"), DRM_ERR_ARG),
             (field(3, "1.5"), DRM_ERR_ARG), (field(3, "-1"), DRM_ERR_ARG), (field(3, str(2 ** 31)), DRM_ERR_ARG),
             (field(4, "256"), DRM_ERR_ARG), (field(7, "a"), DRM_ERR_ARG), (field(8, "1e3"), DRM_ERR_ARG),
             (field(5, "4"), DRM_ERR_ARG), (field(5, "M"), DRM_ERR_ARG), (field(5, "4Q"), DRM_ERR_ARG),
             (field(5, "4M3"), DRM_ERR_ARG), (field(5, ""), DRM_ERR_ARG),
             (field(10, "III"), DRM_ERR_ARG), (field(10, "IIIII"), DRM_ERR_ARG),
             (field(2, "chr9"), DRM_ERR_ARG), (field(6, "chr9"), DRM_ERR_ARG),
             (ok + "\tNM:i:x", DRM_ERR_ARG), (ok + "\tNM:i:" + str(2 ** 32), DRM_ERR_ARG), (ok + "\tNM", DRM_ERR_ARG),
             (ok + "\tXT:A:UU", DRM_ERR_ARG),
             (ok + "\tXF:f:1.5", DRM_ERR_UNSUPPORTED), (ok + "\tXB:B:c,1", DRM_ERR_UNSUPPORTED),
             (ok + "\tXH:H:1AE3", DRM_ERR_UNSUPPORTED),
             (field(0, "q" * 255), DRM_ERR_UNSUPPORTED)]
    for line, code in cases:
        with pytest.raises(DrmError) as e:
            bam_record(line, NAMES)
        assert e.value.code == code, (line, str(e.value))
    with pytest.raises(DrmError) as e:
        bam_record(field(2, "chr1"), [])
    assert e.value.code == DRM_ERR_ARG
    assert bam_record(field(2, "*"), []) == B.encode_record(field(2, "*"), [])


def test_header_equals_the_python_restatement():
    from deepreadmapper_amd import DrmError, bam_header
    one = "@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:ref\tLN:150\n"
    four = "@HD\tVN:1.0\tSO:coordinate\n" + "".join(f"@SQ\tSN:chr{c}\tLN:{n}\n" for c, n in
                                                  zip("ABCD", (1000, 2 ** 31 - 1, 1, 77777)))
    for text in (one, four, "", "@HD\tVN:1.0\n", "@SQ\tLN:5\tSN:late\tM5:x\n@CO\t@SQ\tSN:no\tLN:1\n"):
        assert bam_header(text) == B.encode_header(text), text
    assert bam_header(one)[-4 - 4 - 4 - 4:] == struct.pack("<II", 1, 4) + b"ref\0" + struct.pack("<I", 150)
    assert B.decode_bam(bam_header(four)) == four.split("\n")[:-1]
    for text in ("@SQ\tSN:a\n", "@SQ\tLN:4\n", "@SQ\tSN:a\tLN:x\n", "@SQ\tSN:a\tLN:-4\n"):
        with pytest.raises(DrmError):
            bam_header(text)
    big = "@CO\t" + "x" * 10000 + "\n" + one  # larger than the wrapper's first buffer
    assert bam_header(big) == B.encode_header(big)


def test_a_whole_file_of_records_decodes_to_its_lines():
    from deepreadmapper_amd import bam_header, bam_record
    text = "@HD\tVN:1.0\tSO:unsorted\n" + "".join(f"@SQ\tSN:{n}\tLN:700000000\n" for n in NAMES)
    lines = [LINES[k] for k in sorted(LINES) if k != "base_outside_the_alphabet"]  # which decodes to another letter
    raw = bam_header(text) + b"".join(bam_record(x, NAMES) for x in lines)
    assert B.decode_bam(raw) == text.split("\n")[:-1] + lines


def test_fixed_numbers_and_argument_errors_that_touch_no_device():
    from deepreadmapper_amd import DrmError, bgzf_block, bgzf_bound, bgzf_compress, bgzf_eof, bgzf_workspace
    from deepreadmapper_amd._native import DRM_ERR_ARG, lib
    import ctypes as C
    assert bgzf_block() == B.BLOCK == 0xff00
    assert [bgzf_bound(n) for n in (0, 1, 65280, 65281, 3 * 65280)] == [0, 32, 65311, 65343, 3 * 65311]
    assert bgzf_eof() == B.EOF and len(B.EOF) == 28
    assert B.read_bgzf(bgzf_eof()) == (b"", [1], [0])
    assert bgzf_compress(b"") == b"" and bgzf_workspace(0) == 0
    got = C.c_size_t(7)
    buf = (C.c_uint8 * 64)()
    L = lib()
    for args in ((None, 5, 0, buf, 64, C.byref(got)), (buf, 5, 0, None, 64, C.byref(got)),
                 (buf, -1, 0, buf, 64, C.byref(got)), (buf, 5, 0, buf, 35, C.byref(got)),
                 (buf, 5, -1, buf, 64, C.byref(got)), (buf, 5, 0, buf, 64, None)):
        assert L.drm_bgzf_compress(*args) == DRM_ERR_ARG, args
    assert L.drm_bgzf_compress(None, 0, 0, None, 0, C.byref(got)) == 0 and got.value == 0
    for args in ((None, 5, buf, buf, buf, 1 << 30, None), (buf, 5, None, buf, buf, 1 << 30, None),
                 (buf, 5, buf, None, buf, 1 << 30, None), (buf, 5, buf, buf, None, 1 << 30, None),
                 (buf, 5, buf, buf, buf, 1000, None), (buf, -5, buf, buf, buf, 1 << 30, None)):
        assert L.drm_bgzf_compress_device(*args) == DRM_ERR_ARG, args
    assert L.drm_bgzf_compress_device(None, 0, None, None, None, 0, None) == 0
    with pytest.raises(DrmError):
        bgzf_bound(-1)


# ----------------------------------------------------------------------------------------- bin/pipeline's option
@pytest.fixture(scope="module")
def option_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_options")
    (d / "idx").mkdir()
    (d / "idx" / "config.txt").write_text("ref_len: 150\nstride: 1\n")
    (d / "sparse").mkdir()
    (d / "sparse" / "config.txt").write_text("ref_len: 150\nstride: 10\n")
    (d / "m1.fastq").write_text("@r0\nACGT\n+\nIIII\n")
    return d


@pytest.mark.parametrize("env,argv", [
    (dict(DRM_SAM_FORMAT=""), {}), (dict(DRM_SAM_FORMAT="BAM"), {}), (dict(DRM_SAM_FORMAT="cram"), {}),
    (dict(DRM_SAM_FORMAT="1"), {}),
    (dict(DRM_SAM_FORMAT="bam", DRM_SAM_CIGAR=None), {}),
    (dict(DRM_SAM_FORMAT="bam"), {9: "0"}), (dict(DRM_SAM_FORMAT="bam"), {8: "0"}),
    (dict(DRM_SAM_FORMAT="bam", DRM_DEVICES="0,0"), {}),
    (dict(DRM_SAM_FORMAT="bam"), {1: "sparse"}),                       # a sparse index's header-only SAM
    (dict(DRM_SAM_FORMAT="bam", DRM_SAM_L2_ROWS="1"), {1: "sparse"}),
], ids=["empty", "upper", "cram", "one", "no_cigar", "not_streaming", "not_dynamic", "two_devices", "header_only",
        "l2_rows"])
def test_pipeline_refuses_the_switch_before_the_index_is_loaded(option_dir, env, argv):
    args = [os.path.join(ROOT, "bin", "pipeline"), "idx", "m1.fastq", "g.fna", "128", "4", "4", "out", "1", "1"]
    for i, v in argv.items():
        args[i] = v
    e = {k: v for k, v in os.environ.items() if not k.startswith("DRM_")}
    e.update({k: v for k, v in {"DRM_SAM_CIGAR": "1", **env}.items() if v is not None})
    r = subprocess.run(args, cwd=option_dir, env=e, capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and "DRM_SAM_FORMAT" in r.stderr, r.stderr
    assert "Index loaded" not in r.stdout and not (option_dir / "out").exists()


def test_pipeline_takes_sam_as_the_default(option_dir):
    """DRM_SAM_FORMAT=sam passes the option check: the run goes on to the index, which this directory cannot serve."""
    args = [os.path.join(ROOT, "bin", "pipeline"), "idx", "m1.fastq", "g.fna", "128", "4", "4", "out", "1", "1"]
    e = {k: v for k, v in os.environ.items() if not k.startswith("DRM_")}
    r = subprocess.run(args, cwd=option_dir, env=dict(e, DRM_SAM_CIGAR="1", DRM_SAM_FORMAT="sam"), capture_output=True,
                       text=True)
    assert r.returncode == 1 and "DRM_SAM_FORMAT" not in r.stderr
