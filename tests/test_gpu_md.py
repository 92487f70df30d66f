"""GPU tests of the MD pass (sw_md.hip, drm_sw_align_md): the words, n_words and the four counts of every pair equal
the plain restatement (tests/md_ref.py) -- on hand-built records and words, which reach the kernel's edges whatever
an aligner emits, on the output of both aligners over a genome and a window table, and on records that describe no
walk (status 3); the truncation rule (status 2) and the device entry point."""
import numpy as np
import pytest

import md_ref as MD
import sw_align_affine_ref as A
import sw_align_ref as R

pytestmark = pytest.mark.gpu

ACGT = list(b"ACGT")
OTHER = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}


def _w(n, op):
    return (n << 4) | op


def _rand(rng, n):
    return bytes(rng.choice(ACGT, size=n).astype(np.uint8))


def _table(windows):
    from deepreadmapper_amd import WindowTable
    return WindowTable(np.frombuffer(b"".join(windows), dtype=np.uint8).reshape(len(windows), len(windows[0])))


def _records(recs):
    from deepreadmapper_amd import SW_ALIGNMENT_DTYPE
    out = np.zeros(len(recs), dtype=SW_ALIGNMENT_DTYPE)
    for p, r in enumerate(recs):
        out[p] = tuple(int(r[f]) for f in R.FIELDS)
    return out


def _assert_equal(h, words, p, region, query, rec, ops):
    want, wwords = MD.md_words(region, query, rec, ops)
    got = {f: int(h[f][p]) for f in MD.MD_FIELDS}
    assert got == want, (p, got, want)
    assert [int(x) for x in words[p]] == wwords, p
    return want


def _walk(rng, region, ops, ref_begin, q_begin, mismatch_at=()):
    """A query and a record for `ops` walked over `region` from ref_begin: M columns copy the region byte except
    the columns (counted along the region from ref_begin) in mismatch_at, I operations add random bases."""
    q = list(_rand(rng, q_begin))
    i = ref_begin
    for x in ops:
        n, op = x >> 4, x & 15
        if op == R.M:
            q += [OTHER[region[c]] if c - ref_begin in mismatch_at else region[c] for c in range(i, i + n)]
        if op == R.I:
            q += list(_rand(rng, n))
        if op != R.I:
            i += n
    rec = dict(dict.fromkeys(R.FIELDS, 0), score=1, ref_begin=ref_begin, ref_end=i, q_begin=q_begin, q_end=len(q),
               n_ops=len(ops))
    return bytes(q), rec


def _hand_cases(rng):
    """(name, ops, ref_begin, q_begin, mismatch columns) over 256-byte windows."""
    for span in (1, 63, 64, 65, 255, 256):  # one operation; a mismatch in the first and in the last column
        yield f"{span} columns", [_w(span, R.M)], (256 - span) // 2, 0, {0, span - 1}
        yield f"{span} columns, exact", [_w(span, R.M)], 256 - span, 0, set()
    # the longest list of the alternating pattern that fits 256 x 256: 85 x (1M 1I 1M 1D) = 340 operations, 255 columns
    yield "340 operations", [_w(1, R.M), _w(1, R.I), _w(1, R.M), _w(1, R.D)] * 85, 1, 0, {0, 7, 100, 168}
    # the maximum of 512 operations: no walk over 256 + 256 bytes has room for an M among that many
    yield "512 operations", [_w(1, R.I), _w(1, R.D)] * 256, 0, 0, set()
    yield "one D of 200", [_w(20, R.M), _w(200, R.D), _w(20, R.M)], 8, 3, {19, 220}
    yield "D I D", [_w(5, R.M), _w(2, R.D), _w(3, R.I), _w(2, R.D), _w(5, R.M)], 100, 1, set()
    yield "every column a mismatch", [_w(256, R.M)], 0, 0, set(range(256))
    yield "runs across insertions", [_w(70, R.M), _w(4, R.I), _w(70, R.M), _w(1, R.I), _w(60, R.M)], 30, 2, {69, 70, 199}
    yield "I at both ends", [_w(3, R.I), _w(64, R.M), _w(2, R.I)], 64, 0, {31}
    yield "adjacent D operations", [_w(10, R.M), _w(2, R.D), _w(3, R.D), _w(10, R.M)], 0, 0, {10 + 5}


def test_hand_built_records_and_words():
    from deepreadmapper_amd import sw_align_md_arrays
    rng = np.random.default_rng(5)
    cases = list(_hand_cases(rng))
    windows = [_rand(rng, 256) for _ in cases]
    queries, recs, ops = [], [], []
    for (name, o, rb, qb, mm), w in zip(cases, windows):
        q, rec = _walk(rng, w, o, rb, qb, mm)
        assert len(q) <= 256 and rec["ref_end"] <= 256, name
        queries.append(q)
        recs.append(rec)
        ops.append(o)
    t = _table(windows)
    ids, pq = np.arange(len(cases)), np.arange(len(cases))
    h, words = sw_align_md_arrays(t, ids, pq, queries, _records(recs), ops)
    h1, words1 = sw_align_md_arrays(t, ids, pq, queries, _records(recs), ops, md_stride=1)
    h513, words513 = sw_align_md_arrays(t, ids, pq, queries, _records(recs), ops, md_stride=513)
    t.free()
    n_words = {}
    for p, (name, *_x) in enumerate(cases):
        want = _assert_equal(h, words, p, windows[p], queries[p], recs[p], ops[p])
        _assert_equal(h1, words1, p, windows[p], queries[p], recs[p], ops[p])
        _assert_equal(h513, words513, p, windows[p], queries[p], recs[p], ops[p])
        assert want["status"] == 0, name
        n_words[name] = want["n_words"]
    assert n_words["every column a mismatch"] == 513 and n_words["512 operations"] == 513
    assert n_words["256 columns, exact"] == 1 and n_words["1 columns"] == 3
    did = [c[0] for c in cases].index("D I D")  # 5M from column 100, then the two deletions
    assert MD.md_string(words[did], 0) \
        == "5^" + windows[did][105:107].decode() + "0^" + windows[did][107:109].decode() + "5"


# ------------------------------------------------------------------------------------------ aligner output
def _mutated_read(rng, w, n):
    """n bytes of window w (from a random start) with substitutions and, for the longer ones, an insertion and a
    deletion, tagged like format_fastq."""
    at = int(rng.integers(0, len(w) - n + 1))
    s = list(w[at:at + n])
    for _ in range(int(rng.integers(0, 4))):
        s[int(rng.integers(len(s)))] = int(rng.choice(ACGT))
    if n >= 60 and rng.integers(3) == 0:
        x = int(rng.integers(10, len(s) - 10))
        del s[x:x + int(rng.integers(1, 4))]
    if n >= 60 and rng.integers(3) == 0:
        x = int(rng.integers(10, len(s) - 10))
        s[x:x] = [int(c) for c in rng.choice(ACGT, size=int(rng.integers(1, 3)))]
    return b"<" + bytes(s) + b">"


@pytest.fixture(scope="module")
def genome_pairs():
    """2,000 pairs over a 4 kb genome of 150-byte windows: even and odd ids, windows at both genome ends, where a
    flanked region is clamped, a window past the end, and read lengths mixed between 30 and 150 so that a short
    pair follows a long one in the same block."""
    rng = np.random.default_rng(31)
    g = np.frombuffer(_rand(rng, 4000), dtype=np.uint8).copy()
    g[1000:1004] = ord("N")
    gb = bytes(g)
    last = 2 * (len(g) - 150)
    edge = [0, 1, 2, 3, 20, 21, last, last + 1, last - 2, last - 1, last - 40, last - 39, last + 2, last + 3, 2 ** 40]
    wid = np.array(edge + [int(x) for x in rng.integers(0, last + 2, size=2000 - len(edge))], dtype=np.uint64)
    wid[100] = 2 * 930  # a window that holds the Ns
    nq = 400
    lens = [int(x) for x in rng.integers(30, 151, size=nq)]
    lens[0:4] = [150, 30, 150, 31]
    pq = (np.arange(len(wid)) % nq).astype(np.int64)
    queries = [None] * nq
    for p in range(len(wid) - 1, -1, -1):  # query i is cut from the window of the first pair that uses it
        w = R.window_bytes(gb, 150, int(wid[p]))
        if w:
            queries[pq[p]] = _mutated_read(rng, w, lens[pq[p]])
    queries = [q if q is not None else b"<" + _rand(rng, 40) + b">" for q in queries]
    for i in range(4, 8):  # a substitution every 13 bases: more than 16 MD words, so the stride-16 pass truncates
        s = bytearray(R.window_bytes(gb, 150, int(wid[i])))
        for c in range(6, 150, 13):
            s[c] = OTHER[s[c]]
        queries[i] = b"<" + bytes(s) + b">"
    return {"g": g, "gb": gb, "wid": wid, "pq": pq, "queries": queries}


@pytest.mark.parametrize("flank,scoring", [(0, (1, 4, 6, 1)), (32, (1, 4, 6, 1)), (32, (2, 4, 4, 2))])
def test_affine_aligner_output_on_a_genome(genome_pairs, flank, scoring):
    """The 2,000 pairs three times over in one call: 6,000 pairs are more than the launch's blocks, so the grid-stride
    loop runs and a block meets long and short pairs in turn."""
    from deepreadmapper_amd import GenomeTable, sw_align_affine_arrays, sw_align_md_arrays
    d = genome_pairs
    wid, pq = np.tile(d["wid"], 3), np.tile(d["pq"], 3)
    t = GenomeTable(d["g"], 150)
    rec, ops = sw_align_affine_arrays(t, wid, pq, d["queries"], scoring, flank=flank)
    h, words = sw_align_md_arrays(t, wid, pq, d["queries"], rec, ops, flank=flank)
    t.free()
    n = len(d["wid"])
    statuses, longest = set(), 0
    for p in range(n):
        region = A.region_bytes(d["gb"], 150, int(wid[p]), flank)
        want = _assert_equal(h, words, p, region, d["queries"][pq[p]], rec[p], ops[p])
        statuses.add(want["status"])
        longest = max(longest, want["n_words"])
        if want["status"] == 0:
            assert want["n_mismatch"] + want["n_ins"] + want["n_del"] == int(rec["nm"][p]), p
    assert statuses == {0, 1} and longest > 16  # some pairs went through the retry at the full stride
    for rep in (1, 2):
        assert h[rep * n:(rep + 1) * n].tobytes() == h[:n].tobytes()
        assert all(np.array_equal(words[rep * n + p], words[p]) for p in range(n))


def test_linear_aligner_output_on_a_genome_and_on_a_window_table(genome_pairs):
    from deepreadmapper_amd import GenomeTable, sw_align_arrays, sw_align_md_arrays
    d = genome_pairs
    t = GenomeTable(d["g"], 150)
    rec, ops = sw_align_arrays(t, d["wid"], d["pq"], d["queries"])
    h, words = sw_align_md_arrays(t, d["wid"], d["pq"], d["queries"], rec, ops)
    t.free()
    for p in range(len(d["wid"])):
        want = _assert_equal(h, words, p, R.window_bytes(d["gb"], 150, int(d["wid"][p])), d["queries"][d["pq"][p]],
                             rec[p], ops[p])
        assert want["status"] == 1 or want["n_mismatch"] + want["n_ins"] + want["n_del"] == int(rec["nm"][p])
    # a window table: rows are the windows, ids past the table are empty
    rng = np.random.default_rng(32)
    windows = [R.window_bytes(d["gb"], 150, int(x)) for x in rng.integers(0, 2 * 3800, size=64)]
    queries = [_mutated_read(rng, w, int(rng.integers(30, 151))) for w in windows]
    wid = np.array(list(range(64)) * 4 + [64, 2 ** 40 + 1], dtype=np.uint64)
    pq = np.array(list(range(64)) * 4 + [0, 1], dtype=np.int64)
    pq[64:128] = (pq[64:128] + 1) % 64  # a read against a foreign window: short or no alignments
    t = _table(windows)
    rec, ops = sw_align_arrays(t, wid, pq, queries)
    h, words = sw_align_md_arrays(t, wid, pq, queries, rec, ops)
    t.free()
    for p in range(len(wid)):
        region = windows[int(wid[p])] if int(wid[p]) < 64 else b""
        want = _assert_equal(h, words, p, region, queries[pq[p]], rec[p], ops[p])
        assert want["status"] == 1 or want["n_mismatch"] + want["n_ins"] + want["n_del"] == int(rec["nm"][p])
    assert [int(x) for x in h["status"][-2:]] == [1, 1] and (h["status"][:64] == 0).all()


# ------------------------------------------------------------------------------------------ status 1, 2, 3
def _twenty_word_case(rng):
    """A 150-column walk with 8 mismatches and one D of 2: 8 * 2 + 1 + 2 + 1 = 20 words."""
    w = _rand(rng, 150)
    o = [_w(80, R.M), _w(2, R.D), _w(68, R.M)]
    q, rec = _walk(rng, w, o, 0, 1, {3, 9, 10, 40, 79, 82, 120, 149})
    return w, q, rec, o


def test_status_2_stores_the_first_words_and_the_retry_returns_all():
    from deepreadmapper_amd import SW_MD_DTYPE, sw_align_md_arrays
    from deepreadmapper_amd import rerank as RR
    from deepreadmapper_amd._native import check, lib
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    rng = np.random.default_rng(8)
    w, q, rec, o = _twenty_word_case(rng)
    want, wwords = MD.md_words(w, q, rec, o)
    assert want["n_words"] == 20
    t = _table([w, w])
    # pair 1 has no alignment: its row, behind pair 0's, must stay as it was
    recs = _records([rec, dict(dict.fromkeys(R.FIELDS, 0), status=1)])
    qbuf, qlen = RR.pack_queries([q])
    d = [DeviceBuffer.from_host(x) for x in (np.array([0, 1], dtype=np.uint64), np.array([0, 0], dtype=np.int64), qbuf,
                                             qlen, recs, np.array(o, dtype=np.uint32), np.zeros(2, dtype=np.int64))]
    d_h = DeviceBuffer(2, SW_MD_DTYPE)
    d_md = DeviceBuffer.from_host(np.full((3, 16), 0xFFFFFFFF, dtype=np.uint32))
    st = Stream()
    check(lib().drm_sw_align_md_device(t.handle, 0, d[0].ptr, d[1].ptr, 2, d[2].ptr, d[3].ptr, qbuf.shape[1], 1,
                                       d[4].ptr, d[5].ptr, d[6].ptr, d_h.ptr, d_md.ptr, 16, st.handle))
    st.synchronize()
    h, md = d_h.download(), d_md.download()
    assert [int(x) for x in h[0]] == [20, want["n_match"], 8, 0, 2, 2]
    assert [int(x) for x in h[1]] == [0, 0, 0, 0, 0, 1]
    assert [int(x) for x in md[0]] == wwords[:16]
    assert (md[1:] == 0xFFFFFFFF).all()
    h2, words = sw_align_md_arrays(t, [0, 1], [0, 0], [q], recs, [o, []])
    t.free()
    assert [int(x) for x in h2[0]] == [20, want["n_match"], 8, 0, 2, 0] and [int(x) for x in words[0]] == wwords
    assert int(h2["status"][1]) == 1 and len(words[1]) == 0


def test_status_3_for_each_inconsistency_between_valid_neighbours():
    from deepreadmapper_amd import sw_align_md_arrays
    rng = np.random.default_rng(9)
    w, q, good, o = _twenty_word_case(rng)  # spans 150 region bytes and 148 query bytes from (0, 1)
    short = bytes(rng.choice(ACGT, size=100).astype(np.uint8))  # a query shorter than the record's q_end
    bad = [
        ("record status 2", dict(good, status=2), o),
        ("record status 7", dict(good, status=7), o),
        ("n_ops 0", dict(good, n_ops=0), o),
        ("n_ops negative", dict(good, n_ops=-3), o),
        ("n_ops 513", dict(good, n_ops=513), o),
        ("n_ops 2^30", dict(good, n_ops=1 << 30), o),
        ("kind 3", good, [o[0], _w(2, 3), o[2]]),
        ("kind 15", good, [o[0], _w(2, 15), o[2]]),
        ("zero length", dict(good, n_ops=4), o + [_w(0, R.M)]),
        ("negative ref_begin", dict(good, ref_begin=-4, ref_end=146), o),
        ("negative q_begin", dict(good, q_begin=-1, q_end=147), o),
        ("ref_begin > ref_end", dict(good, ref_begin=100, ref_end=50), o),
        ("ref_end past the region", dict(good, ref_begin=1, ref_end=151), o),
        ("q_begin > q_end", dict(good, q_begin=120, q_end=20), o),
        ("q_end past the query", dict(good, q_begin=5, q_end=153), o),
        ("reference span", dict(good, ref_end=149), o),
        ("query span", dict(good, q_end=148), o),
        ("a length of 2^27", good, [o[0], _w(1 << 27, R.D), o[2]]),
        # 32 * (2^27 + 4) = 2^32 + 128: summed in 32 bits without a cap the spans would come out right
        ("lengths that wrap 32 bits", dict(good, n_ops=34), [_w((1 << 27) + 4, R.M)] * 32 + [_w(2, R.D), _w(20, R.M)]),
    ]
    recs, ops, qsel = [good], [o], [0]
    for name, r, words in bad:
        recs += [r, good]
        ops += [words, o]
        qsel += [0, 0]
    recs += [dict(good), good]  # q_end past a shorter query, then a valid pair
    ops += [o, o]
    qsel += [1, 0]
    t = _table([w])
    h, words = sw_align_md_arrays(t, np.zeros(len(recs), dtype=np.uint64), qsel, [q, short], _records(recs), ops)
    t.free()
    want, wwords = MD.md_words(w, q, good, o)
    for p in range(len(recs)):
        query = [q, short][qsel[p]]
        res = _assert_equal(h, words, p, w, query, recs[p], ops[p])
        assert res["status"] == (0 if p % 2 == 0 else 3), (p, (bad + [("q_end past a shorter query",)])[p // 2][0])
        if p % 2 == 0:
            assert [int(x) for x in words[p]] == wwords


def test_status_1_records_and_empty_sides():
    from deepreadmapper_amd import GenomeTable, sw_align_md_arrays
    rng = np.random.default_rng(10)
    g = _rand(rng, 600)
    q = b"<" + g[100:250] + b">"
    rec = dict(dict.fromkeys(R.FIELDS, 0), score=150, ref_begin=0, ref_end=150, q_begin=1, q_end=151, n_ops=1)
    none = dict(dict.fromkeys(R.FIELDS, 0), status=1)
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    past = 2 * (600 - 150) + 2
    one = [_w(150, R.M)]
    h, words = sw_align_md_arrays(t, [200, 200, past, 200, 201], [0, 0, 0, 1, 0], [q, b""],
                                  _records([rec, none, rec, rec, rec]), [one, [], one, one, one])
    t.free()
    assert [int(x) for x in h["status"]] == [0, 1, 1, 1, 0]
    assert [int(x) for x in words[0]] == [150 << 4] and all(len(words[p]) == 0 for p in (1, 2, 3))
    assert int(h["n_mismatch"][4]) > 50  # the reverse strand of the same place: the walk is taken as given
    for p in (1, 2, 3):
        assert [int(x) for x in h[p]] == [0, 0, 0, 0, 0, 1]


# ------------------------------------------------------------------------------------------ device entry point
def test_device_entry_point_on_a_stream_equals_the_host_form(genome_pairs):
    from deepreadmapper_amd import SW_MD_DTYPE, GenomeTable, sw_align_affine_arrays
    from deepreadmapper_amd import rerank as RR
    from deepreadmapper_amd._native import check, lib
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    d = genome_pairs
    n, flank = 600, 32
    wid, pq = d["wid"][:n].copy(), d["pq"][:n].copy()
    t = GenomeTable(d["g"], 150)
    rec, ops = sw_align_affine_arrays(t, wid, pq, d["queries"], (1, 4, 6, 1), flank=flank)
    qbuf, qlen = RR.pack_queries(d["queries"])
    off = np.zeros(n, dtype=np.int64)
    off[1:] = np.cumsum([len(o) for o in ops[:-1]])
    flat = np.concatenate([np.asarray(o, dtype=np.uint32) for o in ops] + [np.zeros(1, dtype=np.uint32)])
    stride = 2 * (150 + 2 * flank) + 1
    h = np.zeros(n, dtype=SW_MD_DTYPE)
    md = np.zeros((n, stride), dtype=np.uint32)
    check(lib().drm_sw_align_md(t.handle, flank, RR.ptr(wid), RR.ptr(pq), n, RR.ptr(qbuf), RR.ptr(qlen), qbuf.shape[1],
                                len(qlen), RR.ptr(rec), RR.ptr(flat), RR.ptr(off), RR.ptr(h), RR.ptr(md), stride))
    # the device form cannot refuse a query index outside [0, nq): such a pair has an empty query, status 1
    dpq = pq.copy()
    dpq[[50, 51]] = [len(qlen), -1]
    dev = [DeviceBuffer.from_host(x) for x in (wid, dpq, qbuf, qlen, rec, flat, off)]
    d_h, d_md = DeviceBuffer(n, SW_MD_DTYPE), DeviceBuffer((n, stride), np.uint32)
    d_md.zero()
    st = Stream()
    check(lib().drm_sw_align_md_device(t.handle, flank, dev[0].ptr, dev[1].ptr, n, dev[2].ptr, dev[3].ptr,
                                       qbuf.shape[1], len(qlen), dev[4].ptr, dev[5].ptr, dev[6].ptr, d_h.ptr, d_md.ptr,
                                       stride, st.handle))
    st.synchronize()
    t.free()
    gh, gmd = d_h.download(), d_md.download()
    ok = np.ones(n, bool)
    ok[[50, 51]] = False
    assert (h["status"][ok] == 0).sum() > 500 and int(rec["status"][50]) == 0 and int(rec["status"][51]) == 0
    assert gh[ok].tobytes() == h[ok].tobytes() and gmd[ok].tobytes() == md[ok].tobytes()
    assert [tuple(int(x) for x in r) for r in gh[~ok]] == [(0, 0, 0, 0, 0, 1)] * 2 and not gmd[~ok].any()
