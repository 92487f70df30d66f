"""GPU tests of the mate rescue (mate_rescue.hip, drm_mate_rescue / drm_mate_rescue_device): every field of every
record equals the Python restatement of the definition (tests/mate_rescue_ref.py). Where a rescue region coincides with
a flanked window the affine alignment kernel is a second oracle; regions past the aligners' 256 rows, every query
shape of both builds, the tie rule, the largest score, the empty cases, more tasks than launched waves, the device
form, the hand-off to the aligners and the chain pair_hits -> mate_rescue -> pair_rescue_choose follow."""
import numpy as np
import pytest

import mate_rescue_ref as M
import pair_ref as P
import sw_align_affine_ref as A
import sw_align_ref as R
from deepreadmapper_amd import mate_rescue, pair_rescue_choose  # noqa: F401  (what this file is about)
from test_gpu_sw_align_affine import _edited_reads, _mutated_query, _rand

pytestmark = pytest.mark.gpu

ACGT = list(b"ACGT")
LINEAR = (1, 1, 0, 1)
SCORINGS = [LINEAR, (1, 4, 6, 1), (2, 4, 4, 2)]


def F(pos):
    return 2 * pos


def Rv(pos):
    return 2 * pos + 1


def _genome_table(g, ref_len):
    from deepreadmapper_amd import GenomeTable
    return GenomeTable(np.frombuffer(bytes(g), dtype=np.uint8), ref_len)


def _oriented(read, rev):
    """The query that matches genome bytes `read` in a region of orientation rev, tagged as the CLI tags reads."""
    return b"<" + (R.revcomp(read) if rev else bytes(read)) + b">"


def _rescue(t, g, anchors, tq, queries, scoring=LINEAR, mn=0, mx=1000, what=""):
    """The package's records of a task list equal the restatement's on every field; returns them as dicts."""
    from deepreadmapper_amd import mate_rescue
    got = mate_rescue(t, anchors, tq, queries, mn, mx, scoring)
    cache = {}
    want = []
    for w, q in zip(anchors, tq):
        key = (int(w), int(q))
        if key not in cache:
            cache[key] = M.rescue_one(g, t.ref_len, int(w), queries[int(q)], scoring, mn, mx)
        want.append(cache[key])
    M.assert_equal(got, want, what)
    return want


# ------------------------------------------------------------------------------------------ 1. the affine kernel as oracle
# (ref_len, flank): region lengths 1, 2, 3, 63, 64, 65, 166, 255, 256
ORACLE_SHAPES = [(1, 0), (2, 0), (1, 1), (33, 15), (64, 0), (33, 16), (150, 8), (255, 0), (150, 53), (256, 0)]


@pytest.mark.parametrize("ref_len,flank", ORACLE_SHAPES)
def test_region_of_a_flanked_window_equals_the_affine_kernel(ref_len, flank):
    """dlo = d, dhi = d + 2 * flank: the region of forward anchor a is that of window 2 * (a + d + flank) + 1 at that
    flank, the region of reverse anchor a that of window 2 * (a - d - flank)."""
    from deepreadmapper_amd import mate_rescue, mate_rescue_region, sw_align_affine_arrays, sw_align_region
    rng = np.random.default_rng(100 * ref_len + flank)
    g = _rand(rng, 1500)
    t = _genome_table(g, ref_len)
    n = ref_len + 2 * flank
    lens = sorted({1, 2, min(n, 5), min(n + 2, 64), min(n + 2, 152), min(n + 2, 193), min(n + 2, 256)})
    for d in (0, 7):
        mn, mx = d + ref_len, d + 2 * flank + ref_len
        anchors, windows = [], []
        for a in (400, 431):
            anchors += [F(a), Rv(a + 300)]
            windows += [Rv(a + d + flank), F(a + 300 - d - flank)]
        for anchor, w in zip(anchors, windows):
            assert mate_rescue_region(len(g), ref_len, anchor, mn, mx) == sw_align_region(t, w, flank) == \
                M.region(len(g), ref_len, anchor, mn, mx)
            assert sw_align_region(t, w, flank)[1] == n
        for short in (True, False):  # the 3- and the 4-columns-per-lane build
            ql = [x for x in lens if (x <= 192) == short]
            if not ql:
                continue
            queries, tasks = [], []
            for x, (anchor, w) in enumerate(zip(anchors, windows)):
                wb = A.region_bytes(g, ref_len, w, flank)
                for q_len in ql:
                    tasks.append((anchor, w, len(queries)))
                    queries.append(_mutated_query(rng, wb, q_len))
            an = [a for a, _, _ in tasks]
            wi = [w for _, w, _ in tasks]
            tq = [q for _, _, q in tasks]
            for scoring in SCORINGS:
                got = mate_rescue(t, an, tq, queries, mn, mx, scoring)
                rec, _ = sw_align_affine_arrays(t, wi, tq, queries, scoring, flank=flank)
                for f in ("score", "ref_end", "q_end", "status"):
                    assert [int(x) for x in got[f]] == [int(x) for x in rec[f]], (f, d, short, scoring)
                _rescue(t, g, an, tq, queries, scoring, mn, mx, (d, short, scoring))
                assert (got["status"] == 0).sum() >= len(tasks) // 2
    t.free()


# ------------------------------------------------------------------------------------------ 2. past the old limits
@pytest.mark.parametrize("rows", [257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048])
def test_regions_past_256_rows(rows):
    """min_tlen = 0, max_tlen = rows: a region of `rows` rows on either strand; 150-base reads planted so that the end
    cell lies in the first row a whole read can end in, in the last row, and on either side of 512 and 1,024; a
    one-byte query ends in row 1."""
    rng = np.random.default_rng(rows)
    g = _rand(rng, 6000)
    t = _genome_table(g, 150)
    ends = sorted({150, rows} | {r for r in (511, 512, 513, 1023, 1024, 1025) if 150 <= r <= rows})
    for anchor in (F(2000), Rv(4200)):
        s, n, rev = M.region(len(g), 150, anchor, 0, rows)
        assert n == rows
        region = M.region_bytes(g, 150, anchor, 0, rows)
        queries = [b"<" + region[e - 150:e] + b">" for e in ends] + [region[:1]]
        want = _rescue(t, g, [anchor] * len(queries), np.arange(len(queries)), queries, LINEAR, 0, rows, anchor)
        for x, e in enumerate(ends):
            assert (want[x]["score"], want[x]["ref_end"], want[x]["q_end"]) == (150, e, 151), (anchor, e)
        assert (want[len(ends)]["score"], want[len(ends)]["ref_end"], want[len(ends)]["q_end"]) == (1, 1, 1)
    # the same under a scoring whose scores need more than 8 bits beside an 11-bit row
    anchor = F(2000)
    region = M.region_bytes(g, 150, anchor, 0, rows)
    queries = [b"<" + region[e - 150:e] + b">" for e in (150, rows)]
    want = _rescue(t, g, [anchor, anchor], [0, 1], queries, (31, 63, 63, 63), 0, rows)
    assert [w["score"] for w in want] == [31 * 150] * 2 and [w["ref_end"] for w in want] == [150, rows]
    t.free()


# ------------------------------------------------------------------------------------------ 3. query shapes
Q_LENS = [1, 2, 3, 4, 5, 63, 64, 65, 152, 189, 190, 191, 192, 193, 253, 254, 255, 256]


@pytest.mark.parametrize("scoring", SCORINGS)
def test_query_lengths_of_both_builds(scoring):
    """One call per build (the longest query of a call chooses it): 3 columns per lane up to 192 bytes, 4 beyond."""
    rng = np.random.default_rng(31)
    g = _rand(rng, 1200)
    t = _genome_table(g, 150)
    for lens in ([x for x in Q_LENS if x <= 192], Q_LENS):
        anchors, queries = [], []
        for x, q_len in enumerate(lens):
            anchor = F(100 + 3 * x) if x % 2 else Rv(700 + 3 * x)
            region = M.region_bytes(g, 150, anchor, 0, 400)
            at = int(rng.integers(0, len(region) - 256))
            anchors.append(anchor)
            queries.append(_mutated_query(rng, region[at:at + 256], q_len))
        assert [len(q) for q in queries] == lens
        want = _rescue(t, g, anchors, np.arange(len(lens)), queries, scoring, 0, 400, (scoring, len(lens)))
        assert sum(w["status"] == 0 for w in want) >= len(lens) - 2
    t.free()


@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("ref_len", [150, 252])
def test_indels_on_the_lanes_column_boundaries(ref_len, scoring):
    """152-byte reads (3 columns per lane) and 254-byte reads (4 per lane, whose column groups end on 188 to 193), each
    with one edit, an indel's first or last base on a lane's first or last column; the region is the whole genome, on
    either strand."""
    rng = np.random.default_rng(2000 + ref_len)
    g = _rand(rng, ref_len + 250)
    columns =[2, 3, 4, 5, 63, 64, 65, 127, 128, 129] + ([188, 189, 190, 191, 192, 193] if ref_len > 190 else [])
    reads = [q for _, q in _edited_reads(rng, g, ref_len, columns)]
    assert {len(q) for q in reads} == {ref_len + 2}
    t = _genome_table(g, ref_len)
    for anchor in (Rv(len(g) - ref_len), F(0)):
        assert M.region(len(g), ref_len, anchor, 0, len(g)) == (0, len(g), 1 - anchor % 2)
        queries = [_oriented(q[1:-1], 1 - anchor % 2) for q in reads]
        want = _rescue(t, g, [anchor] * len(queries), np.arange(len(queries)), queries, scoring, 0, len(g), anchor)
        assert all(w["status"] == 0 and w["score"] >= scoring[0] * 50 for w in want)
    t.free()


# ------------------------------------------------------------------------------------------ 4. ties
def test_the_smaller_row_wins_in_both_orientations():
    """The same 150 bases at two places of the genome: the copy that comes first in the region as oriented wins."""
    rng = np.random.default_rng(41)
    g = bytearray(_rand(rng, 3000))
    read = bytes(g[1200:1350])
    g[1700:1850] = read
    g = bytes(g)
    t = _genome_table(g, 150)
    # reverse anchor at 2000: the region genome[1000, 2150) as it stands, rows 1-based from genome[1000]
    want = _rescue(t, g, [Rv(2000)], [0], [_oriented(read, 0)], LINEAR, 0, 1150)
    assert (want[0]["score"], want[0]["ref_end"]) == (150, 1350 - 1000)
    # forward anchor at 1000: genome[1000, 2150) reversed, row 1 is genome[2149]: the copy at 1700 comes first
    want = _rescue(t, g, [F(1000)], [0], [_oriented(read, 1)], LINEAR, 0, 1150)
    assert (want[0]["score"], want[0]["ref_end"]) == (150, 2150 - 1700)
    t.free()


def test_the_smaller_column_wins_across_a_lane_boundary():
    """A one-row region 'A': every 'A' of the query scores 1 in row 1. Columns 3 and 4 (lanes 0 and 1 of the
    3-column build), columns 4 and 5 (lanes 0 and 1 of the 4-column build), and a column far to the right."""
    g = b"CCCCACCCC"
    t = _genome_table(g, 1)
    for pad in (0, 200):  # the longest query of the call chooses the build
        queries = [b"CCAACC", b"CCCAAC", b"G" * 17 + b"A" + b"G" * 50 + b"A", b"G" * (56 + pad)]
        want = _rescue(t, g, [Rv(4)] * 3, [0, 1, 2], queries, LINEAR, 1, 1, pad)
        assert [(w["ref_end"], w["q_end"]) for w in want] == [(1, 3), (1, 4), (1, 18)]
        want = _rescue(t, g, [F(4)] * 3, [0, 1, 2], [q.replace(b"A", b"T") for q in queries], LINEAR, 1, 1, pad)
        assert [(w["ref_end"], w["q_end"]) for w in want] == [(1, 3), (1, 4), (1, 18)]
    t.free()


@pytest.mark.parametrize("scoring", SCORINGS)
def test_two_letter_strings_full_of_ties(scoring):
    rng = np.random.default_rng(43)
    g = _rand(rng, 400, list(b"AC"))
    t = _genome_table(g, 16)
    queries = [_rand(rng, int(rng.integers(1, 41)), list(b"ACGT" if i % 2 else b"AC")) for i in range(40)]
    anchors = [F(int(rng.integers(0, 300))) if i % 2 else Rv(int(rng.integers(80, 384))) for i in range(40)]
    want = _rescue(t, g, anchors, np.arange(40), queries, scoring, 0, 64, scoring)
    assert sum(w["status"] == 0 for w in want) >= 30
    t.free()


# ------------------------------------------------------------------------------------------ 5. the largest score
def test_largest_score():
    """256 x A against 2,048 rows of A at match 31: score 31 * 256, the first row that holds it is 256."""
    g = b"A" * 2400
    t = _genome_table(g, 150)
    big = (31, 63, 63, 63)
    want = _rescue(t, g, [Rv(2200), F(100)], [0, 1], [b"A" * 256, b"T" * 256], big, 0, 2048)
    assert [(w["region_len"], w["score"], w["ref_end"], w["q_end"]) for w in want] == [(2048, 31 * 256, 256, 256)] * 2
    t.free()


# ------------------------------------------------------------------------------------------ 6. other cases
def test_n_bases_and_empty_cases():
    rng = np.random.default_rng(61)
    g = bytearray(_rand(rng, 2000))
    g[900:906] = b"N" * 6  # raw byte equality: N matches N, and N is its own complement
    g = bytes(g)
    t = _genome_table(g, 150)
    read = g[830:980]
    last = len(g) - 150
    anchors = [Rv(1200), F(500), F(last), F(last + 1), Rv(last + 1), F(2 ** 40), Rv(2 ** 63 - 1), Rv(0), F(last - 100)]
    queries = [_oriented(read, 0), _oriented(read, 1)] + [_oriented(read, a % 2 == 0) for a in anchors[2:]]
    want = _rescue(t, g, anchors, np.arange(len(anchors)), queries)
    assert [w["score"] for w in want[:2]] == [150, 150]
    assert [w["status"] for w in want[3:7]] == [1] * 4 and [w["region_len"] for w in want[3:7]] == [0] * 4
    assert (want[2]["region_start"], want[2]["region_len"]) == (last, 150)
    assert (want[7]["region_start"], want[7]["region_len"]) == (0, 150)
    # dhi < dlo: max_tlen below ref_len accepts no template length
    want = _rescue(t, g, anchors[:2], [0, 1], queries, LINEAR, 0, 149)
    assert [(w["region_len"], w["status"]) for w in want] == [(0, 1)] * 2
    # a query of which nothing matches
    want = _rescue(t, g, anchors[:2], [0, 0], [b"<>"])
    assert [w["status"] for w in want] == [1, 1] and [w["region_len"] for w in want] == [1000, 1000]
    t.free()


def test_one_row_region():
    g = b"ACGTTGCA"
    t = _genome_table(g, 1)
    anchors = [F(p) for p in range(8)] + [Rv(p) for p in range(8)]
    for q in (b"A", b"<ACGT>", b"TTTT"):
        want = _rescue(t, g, anchors, [0] * 16, [q], (2, 4, 4, 2), 1, 1, q)
        assert all(w["region_len"] == 1 for w in want)
    t.free()


def _grid_waves():
    from deepreadmapper_amd.device import device_props
    return 32 * device_props(0)["cu_count"]  # launch_mate_rescue's grid bound


def test_more_tasks_than_launched_waves():
    """64-row regions of 16 anchors x 8 queries, each combination at many task positions: a wave loops over tasks and
    reuses its LDS."""
    from deepreadmapper_amd import mate_rescue
    rng = np.random.default_rng(5)
    g = _rand(rng, 600)
    t = _genome_table(g, 32)
    anchors = [F(20 + 31 * i) if i % 2 else Rv(90 + 31 * i) for i in range(16)]
    queries = [_mutated_query(rng, M.region_bytes(g, 32, anchors[2 * i], 0, 64), 10 + 6 * i) for i in range(8)]
    want = {(a, q): M.rescue_one(g, 32, anchors[a], queries[q], (1, 4, 6, 1), 0, 64) for a in range(16) for q in range(8)}
    ntasks = _grid_waves() + 37
    combo = (37 * np.arange(ntasks)) % 128
    a, q = combo // 8, combo % 8
    got = mate_rescue(t, np.array(anchors, dtype=np.uint64)[a], q, queries, 0, 64, (1, 4, 6, 1))
    t.free()
    assert len(got) == ntasks
    M.assert_equal(got, [want[(int(a[p]), int(q[p]))] for p in range(ntasks)])
    assert {w["region_len"] for w in want.values()} == {64} and sum(w["status"] == 0 for w in want.values()) > 64


def test_device_form_equals_host_form():
    from deepreadmapper_amd import RESCUE_RESULT_DTYPE, mate_rescue, mate_rescue_device
    from deepreadmapper_amd import rerank as RR
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    rng = np.random.default_rng(17)
    g = _rand(rng, 3000)
    t = _genome_table(g, 150)
    n = 200
    anchors = rng.integers(0, 2 * (len(g) - 150) + 6, size=n).astype(np.uint64)  # a few past the genome end
    queries = [_oriented(g[p:p + 150], (p // 100) % 2) for p in range(500, 2500, 100)]
    tq = (np.arange(n) % len(queries)).astype(np.int64)
    anchors[30] = 2 * (len(g) - 150) + 2  # past the genome end
    tq[7], tq[11] = len(queries), -1  # the device form cannot refuse an index outside [0, nq): status 1
    qbuf, qlen = RR.pack_queries(queries)
    st = Stream()
    d = [DeviceBuffer.from_host(x) for x in (anchors, tq, qbuf, qlen)]
    d_out = mate_rescue_device(t, d[0], d[1], n, d[2], d[3], qbuf.shape[1], len(qlen), 0, 700, (2, 4, 4, 2),
                               stream=st)
    st.synchronize()
    got = d_out.download()
    assert got.dtype == RESCUE_RESULT_DTYPE
    ok = np.ones(n, bool)
    ok[[7, 11]] = False
    want = mate_rescue(t, anchors[ok], tq[ok], queries, 0, 700, (2, 4, 4, 2))
    assert got[ok].tobytes() == want.tobytes()
    assert (want["status"] == 0).sum() > 20 and (want["region_len"] == 0).any()
    for p in (7, 11):
        assert {f: int(got[f][p]) for f in M.FIELDS} == M.rescue_one(g, 150, int(anchors[p]), None, (2, 4, 4, 2), 0, 700)
    for b in d + [d_out]:
        b.free()
    t.free()


def test_argument_errors_leave_the_handle_usable():
    from deepreadmapper_amd import DrmError, WindowTable, mate_rescue
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED
    rng = np.random.default_rng(3)
    g = _rand(rng, 2000)
    genome = _genome_table(g, 150)
    table = WindowTable(np.frombuffer(g[:1500], dtype=np.uint8).reshape(10, 150))
    q = _oriented(g[400:550], 1)

    def code(t, *a, **kw):
        with pytest.raises(DrmError) as e:
            mate_rescue(t, [F(100)], [0], [q], *a, **kw)
        return e.value.code
    assert code(table) == DRM_ERR_ARG  # a window table holds nothing between its rows
    assert code(genome, ref_len=149) == DRM_ERR_ARG  # not the handle's
    assert code(genome, 0, 2049) == DRM_ERR_UNSUPPORTED
    assert code(genome, 10, 5) == DRM_ERR_ARG
    assert code(genome, -1, 5) == DRM_ERR_ARG
    for field, values in enumerate([(0, 32, -1), (0, 64, -1), (-1, 64), (0, 64, -1)]):
        for v in values:
            bad = list(LINEAR)
            bad[field] = v
            assert code(genome, 0, 1000, bad) == DRM_ERR_ARG, (field, v)
    for tq in (1, -1):  # the host form checks the task's query index
        with pytest.raises(DrmError) as e:
            mate_rescue(genome, [F(100)], [tq], [q])
        assert e.value.code == DRM_ERR_ARG
    with pytest.raises(DrmError) as e:
        mate_rescue(genome, [F(100)], [0], [b"A" * 257])
    assert e.value.code == DRM_ERR_UNSUPPORTED
    assert len(mate_rescue(genome, [], [], [q])) == 0
    want = _rescue(genome, g, [F(100)], [0], [q], LINEAR, 0, 2048)  # the cap itself
    assert (want[0]["region_len"], want[0]["score"]) == (1900, 150)
    table.free()
    genome.free()


# ------------------------------------------------------------------------------------------ 7. the hand-off to the aligners
@pytest.mark.parametrize("scoring", [LINEAR, (2, 4, 4, 2)])
def test_the_aligner_finds_the_rescued_hit(scoring):
    """Reads that lack 0, 1, 5 and 12 genome bases, on both strands: drm_sw_align_affine over the window that
    drm_mate_rescue_window names, at flank 16, returns the rescue's score, and its alignment ends (forward region) or
    starts (reversed region) on the genome base the rescue reported."""
    from deepreadmapper_amd import mate_rescue_window, sam_cigar_region, sw_align_affine_arrays, sw_align_region
    rng = np.random.default_rng(71)
    g = _rand(rng, 4000)
    t = _genome_table(g, 150)
    anchors, queries, spans = [], [], []
    for x, nd in enumerate((0, 1, 5, 12)):
        for strand in (0, 1):
            p = 1500 + 37 * x + 11 * strand
            read = g[p:p + 70] + g[p + 70 + nd:p + 150 + nd]  # 150 bases that span 150 + nd of the genome
            assert len(read) == 150
            # the mate of a forward anchor is a reverse hit to its right, that of a reverse anchor a forward hit
            anchors.append(Rv(p + 400) if strand == 0 else F(p - 400))
            queries.append(_oriented(read, strand))
            spans.append((p, p + 150 + nd))
    want = _rescue(t, g, anchors, np.arange(len(anchors)), queries, scoring)
    wr = [mate_rescue_window(w, 150, len(g)) for w in want]
    assert wr == [M.window(w, 150, len(g)) for w in want]
    rec, ops = sw_align_affine_arrays(t, wr, np.arange(len(wr)), queries, scoring, flank=16)
    for x, w in enumerate(want):
        lo, hi = spans[x]
        assert w["status"] == 0 and int(rec["score"][x]) == w["score"], (x, w, rec[x])
        assert wr[x] % 2 == w["reverse"] == x % 2
        start, n, rev = sw_align_region(t, wr[x], 16)
        pos1, _ = sam_cigar_region(rec[x], ops[x], 152, start, n, rev)
        span = int(rec["ref_end"][x]) - int(rec["ref_begin"][x])
        assert (pos1 - 1, pos1 - 1 + span) == (lo, hi), (x, pos1, span)
        if w["reverse"]:  # oriented row ref_end is the alignment's leftmost genome base
            assert pos1 - 1 == w["region_start"] + w["region_len"] - w["ref_end"]
        else:             # ... its last genome base
            assert pos1 - 1 + span - 1 == w["region_start"] + w["ref_end"] - 1
    t.free()


# ------------------------------------------------------------------------------------------ 8. the chain
def rescue_tasks(records):
    """The task list of a block of pair records, as bin/pipeline builds it: (pair, anchor mate, read mate) triples --
    status 1 gives two tasks (the read is mate 2 anchored on mate 1's hit, then mate 1 anchored on mate 2's), status 2
    and 3 one."""
    tasks = []
    for p, r in enumerate(records):
        st = int(r["status"])
        if st in (1, 2):
            tasks.append((p, 0, 1))
        if st in (1, 3):
            tasks.append((p, 1, 0))
    return tasks


def compose_wrappers(t, glen, records, ids, scores, queries, prm, min_score):
    """pair_hits' records of a block (pair p's reads are queries 2p and 2p + 1, ids / scores [2 * npairs, k]) through
    mate_rescue and pair_rescue_choose: [(record dict, rescued window id)] per pair."""
    from deepreadmapper_amd import mate_rescue, pair_rescue_choose
    tasks = rescue_tasks(records)
    chosen = lambda p, m: int(records[p]["j1" if m == 0 else "j2"])  # noqa: E731
    anchors = [int(ids[2 * p + am, chosen(p, am)]) for p, am, _ in tasks]
    res = mate_rescue(t, anchors, [2 * p + rm for p, _, rm in tasks], queries, prm["min_tlen"], prm["max_tlen"], LINEAR)
    by_pair = {}
    for x, (p, am, _) in enumerate(tasks):
        by_pair.setdefault(p, [None, None])[am] = res[x]
    out = []
    for p, r in enumerate(records):
        j = [chosen(p, 0), chosen(p, 1)]
        s = [int(scores[2 * p + m, j[m]]) if j[m] >= 0 else 0 for m in (0, 1)]
        a = [int(ids[2 * p + m, j[m]]) if j[m] >= 0 else 0 for m in (0, 1)]
        rA, rB = by_pair.get(p, [None, None])
        rec, w = pair_rescue_choose(r, s[0], s[1], a[0], a[1], rA, rB, prm["ref_len"], glen, prm["unpaired_penalty"],
                                    min_score)
        out.append(({f: int(rec[f]) for f in M.PAIR_FIELDS}, w))
    return out


def compose_restatement(g, records, ids, scores, queries, prm, min_score):
    """The same from the restatements alone."""
    out = []
    for p, r in enumerate(records):
        j = [r["j1"], r["j2"]]
        s = [int(scores[2 * p + m, j[m]]) if j[m] >= 0 else 0 for m in (0, 1)]
        a = [int(ids[2 * p + m, j[m]]) if j[m] >= 0 else 0 for m in (0, 1)]
        one = lambda am, rm: M.rescue_one(g, prm["ref_len"], a[am], queries[2 * p + rm], LINEAR,  # noqa: E731
                                          prm["min_tlen"], prm["max_tlen"])
        rA = one(0, 1) if r["status"] in (1, 2) else None
        rB = one(1, 0) if r["status"] in (1, 3) else None
        out.append(M.choose(r, s[0], s[1], a[0], a[1], rA, rB, prm["ref_len"], len(g), prm["unpaired_penalty"],
                            min_score))
    return out


def test_chain_pair_hits_rescue_choose():
    """Hand-built hit lists: a proper pair (status 0), pairs whose second / first mate the lists lack (rescued through
    rA / rB), a pair of two unrelated reads (not rescued), pairs with one dead list (status 2 / 3, rescued and not)
    and a pair without hits."""
    from deepreadmapper_amd import pair_hits
    rng = np.random.default_rng(81)
    g = _rand(rng, 8000)
    t = _genome_table(g, 150)
    prm = dict(ref_len=150, min_tlen=0, max_tlen=1000, unpaired_penalty=17)
    k = 4
    fwd = lambda p: _oriented(g[p:p + 150], 0)  # noqa: E731
    rev = lambda p: _oriented(g[p:p + 150], 1)  # noqa: E731
    junk = lambda: b"<" + _rand(rng, 150) + b">"  # noqa: E731
    # (read of mate 1, its rows, read of mate 2, its rows), rows = (window id, score)
    pairs = [
        (fwd(1000), [(F(1000), 150), (F(5000), 90)], rev(1300), [(Rv(1300), 150), (Rv(40), 80)]),   # status 0
        (fwd(2000), [(F(2000), 150)], rev(2400), [(F(6000), 60), (Rv(100), 55)]),                   # 1, through rA
        (fwd(3000), [(Rv(7000), 58), (F(200), 50)], rev(3500), [(Rv(3500), 150)]),                  # 1, through rB
        (junk(), [(F(4000), 70)], junk(), [(F(4500), 65)]),                                          # 1, unrescued
        (rev(5600), [(Rv(5600), 150)], fwd(5100), []),                                               # 2, rescued
        (fwd(600), [(F(600), 150)], junk(), []),                                                     # 2, unrescued
        (rev(6900), [], fwd(6300), [(F(6300), 150)]),                                                # 3, rescued
        (junk(), [], junk(), [(Rv(700), 40)]),                                                       # 3, unrescued
        (junk(), [], junk(), []),                                                                    # 4
    ]
    n = len(pairs)
    ids, scores, cnt = np.zeros((2 * n, k), np.uint64), np.zeros((2 * n, k), np.int32), np.zeros(2 * n, np.int32)
    queries = []
    for p, (q1, h1, q2, h2) in enumerate(pairs):
        for m, (q, h) in enumerate(((q1, h1), (q2, h2))):
            queries.append(q)
            cnt[2 * p + m] = len(h)
            for j, (w, s) in enumerate(h):
                ids[2 * p + m, j], scores[2 * p + m, j] = w, s
    records = pair_hits(ids, scores, cnt, ids[1:], scores[1:], cnt[1:], row_step=2, **prm)
    want_records = P.pair_all(ids, scores, cnt, ids[1:], scores[1:], cnt[1:], row_step=2, **prm)
    P.assert_equal(records, want_records)
    assert [r["status"] for r in want_records] == [0, 1, 1, 1, 2, 2, 3, 3, 4]
    min_score = 60
    got = compose_wrappers(t, len(g), records, ids, scores, queries, prm, min_score)
    t.free()
    assert got == compose_restatement(g, want_records, ids, scores, queries, prm, min_score)
    assert [r["status"] for r, _ in got] == [0, 5, 6, 1, 5, 2, 6, 3, 4]
    assert [w for _, w in got] == [0, Rv(2400), F(3000), 0, F(5100), 0, Rv(6900), 0, 0]
    assert [r["tlen"] for r, _ in got] == [450, 550, 650, 0, 650, 0, 750, 0, 0]
    assert got[1][0]["score"] == 300 and got[2][0]["score"] == 300


def test_device_form_chained_on_pair_hits_device():
    """drm_pair_hits_device and drm_mate_rescue_device on one stream: the pairing's records name the anchors, the
    tasks are uploaded, and the rescue's records equal the host form's."""
    from deepreadmapper_amd import mate_rescue, mate_rescue_device, pair_hits, pair_hits_device
    from deepreadmapper_amd import rerank as RR
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    rng = np.random.default_rng(91)
    g = _rand(rng, 5000)
    t = _genome_table(g, 150)
    n, k = 24, 3
    ids, scores = np.zeros((2 * n, k), np.uint64), np.zeros((2 * n, k), np.int32)
    cnt = np.full(2 * n, k, np.int32)
    queries = []
    for p in range(n):
        a = 300 + 150 * p
        ids[2 * p] = [F(a), F(int(rng.integers(4000))), Rv(int(rng.integers(4000)))]
        scores[2 * p] = [150, 40, 30]
        ids[2 * p + 1] = [F(int(rng.integers(4000))) for _ in range(k)]  # mate 2's true window is not in its list
        scores[2 * p + 1] = [50, 45, 0]
        queries += [_oriented(g[a:a + 150], 0), _oriented(g[a + 350:a + 500], 1)]
    cnt[2 * 5 + 1] = 0  # a pair of status 2
    st = Stream()
    d_ids, d_sc, d_cnt = (DeviceBuffer.from_host(x) for x in (ids, scores, cnt))
    d_pairs = pair_hits_device(d_ids, d_sc, d_cnt, d_ids.ptr + 8 * k, d_sc.ptr + 4 * k, d_cnt.ptr + 4, n, k, 150,
                               row_step=2, stream=st)
    st.synchronize()
    records = d_pairs.download()
    assert records.tobytes() == pair_hits(ids, scores, cnt, ids[1:], scores[1:], cnt[1:], 150, row_step=2).tobytes()
    tasks = rescue_tasks(records)
    assert len(tasks) == 2 * n - 1
    anchors = np.array([ids[2 * p + am, int(records[p]["j1" if am == 0 else "j2"])] for p, am, _ in tasks], np.uint64)
    tq = np.array([2 * p + rm for p, _, rm in tasks], np.int64)
    qbuf, qlen = RR.pack_queries(queries)
    d = [DeviceBuffer.from_host(x) for x in (anchors, tq, qbuf, qlen)]
    d_out = mate_rescue_device(t, d[0], d[1], len(tasks), d[2], d[3], qbuf.shape[1], len(qlen), stream=st)
    st.synchronize()
    got = d_out.download()
    assert got.tobytes() == mate_rescue(t, anchors, tq, queries).tobytes()
    M.assert_equal(got, [M.rescue_one(g, 150, int(a), queries[int(q)]) for a, q in zip(anchors, tq)])
    assert sum(int(got["score"][x]) == 150 for x, (_, am, _) in enumerate(tasks) if am == 0) == n
    for b in [d_ids, d_sc, d_cnt, d_pairs, d_out] + d:
        b.free()
    t.free()
