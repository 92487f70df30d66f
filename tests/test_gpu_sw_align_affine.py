"""GPU tests of the affine-gap alignment over a flanked region (sw_align_affine.hip, drm_sw_align_affine): at
{1, 1, 0, 1} and flank 0 it equals the linear kernel (drm_sw_align) word for word; under other scorings it equals
the Python restatement of the definition (tests/sw_align_affine_ref.py) on every pair; the flank removes the clips
that the window grid and indels cause; drm_sw_align_region and the affine, MD and linear kernels cut one region, and
refuse one row more than 256 alike; the device entry point and the DRM_SAM_SCORING / DRM_SAM_FLANK mode of
bin/pipeline agree with the host form."""
import os
import re
import subprocess

import numpy as np
import pytest

import sw_align_affine_ref as A
import sw_align_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ACGT = list(b"ACGT")
SCORINGS = [(1, 4, 6, 1), (2, 4, 4, 2), (1, 1, 1, 1), (1, 3, 5, 2)]
LINEAR = (1, 1, 0, 1)


def _rand(rng, n, letters=ACGT):
    return bytes(rng.choice(letters, size=n).astype(np.uint8))


def _table(windows):
    from deepreadmapper_amd import WindowTable
    return WindowTable(np.frombuffer(b"".join(windows), dtype=np.uint8).reshape(len(windows), len(windows[0])))


def _check(rec, ops, p, w, q, scoring):
    """Pair p of a wrapper result equals the restatement on (w, q), and its operations replay to its score."""
    want, wops = A.align(w, q, scoring)
    got = {f: int(rec[f][p]) for f in R.FIELDS}
    assert got == want, (p, w, q, scoring, got, want)
    assert [int(x) for x in ops[p]] == wops, (p, w, q, scoring)
    if want["status"] == 0:
        assert A.replay(w, q, rec[p], ops[p], scoring) == (got["score"], got["nm"]), (p, w, q, scoring)


def _mutated_query(rng, w, q_len):
    """A query of exactly q_len bytes from window w: a stretch of it (inside random flanks when the query is longer)
    with a few substitutions, insertions and deletions, tagged like format_fastq when there is room."""
    core = q_len - 2 if q_len >= 3 else q_len
    s = list(w)
    if core < len(s):
        at = int(rng.integers(len(s) - core + 1))
        s = s[at:at + core]
    for _ in range(min(3, len(s) // 8)):
        s[int(rng.integers(len(s)))] = int(rng.choice(ACGT))
    for _ in range(min(2, len(s) // 16)):
        s.insert(int(rng.integers(len(s) + 1)), int(rng.choice(ACGT)))
    for _ in range(min(2, len(s) // 16)):
        del s[int(rng.integers(len(s)))]
    while len(s) < core:
        s.insert(0 if len(s) % 2 else len(s), int(rng.choice(ACGT)))
    s = bytes(s[:core])
    return b"<" + s + b">" if q_len >= 3 else s


def _same(res_a, res_b):
    (ra, oa), (rb, ob) = res_a, res_b
    assert ra.tobytes() == rb.tobytes(), [(p, ra[p], rb[p]) for p in range(len(ra)) if ra[p] != rb[p]][:3]
    assert [list(map(int, x)) for x in oa] == [list(map(int, x)) for x in ob]


# ------------------------------------------------------------------------------------------ 1. the linear kernel as oracle
Q_LENS = [1, 2, 3, 4, 5, 63, 64, 65, 149, 150, 151, 152, 191, 192, 193, 255, 256]


@pytest.mark.parametrize("ref_len", [1, 2, 3, 149, 150, 256])
def test_linear_scoring_equals_the_linear_kernel_on_a_table(ref_len):
    from deepreadmapper_amd import sw_align_affine_arrays, sw_align_arrays
    rng = np.random.default_rng(70 + ref_len)
    windows = [_rand(rng, ref_len) for _ in range(2 * len(Q_LENS))]
    for short in (True, False):  # q_len <= 192 runs the 3-columns-per-lane build, anything longer the 4-column one
        lens = [x for x in Q_LENS if (x <= 192) == short]
        queries = [_mutated_query(rng, windows[2 * a + b], ql) for a, ql in enumerate(lens) for b in range(2)]
        wid = list(range(len(queries))) + [len(windows), 2 ** 40 + 1]  # the last two lie outside the table
        pq = list(range(len(queries))) + [0, 1]
        t = _table(windows)
        lin = sw_align_arrays(t, wid, pq, queries)
        aff = sw_align_affine_arrays(t, wid, pq, queries, LINEAR)
        t.free()
        _same(aff, lin)
        assert [int(s) for s in aff[0]["status"][-2:]] == [1, 1]
        if ref_len >= 149:
            assert {int(x) & 15 for o in aff[1] for x in o} == {R.M, R.I, R.D}


@pytest.mark.parametrize("ref_len", [3, 150])
def test_linear_scoring_equals_the_linear_kernel_on_a_genome(ref_len):
    from deepreadmapper_amd import GenomeTable, sw_align_affine_arrays, sw_align_arrays
    rng = np.random.default_rng(80 + ref_len)
    g = np.frombuffer(_rand(rng, 1200), dtype=np.uint8).copy()
    g[400:406] = ord("N")  # raw byte equality: N matches N, and N is its own complement
    glen = len(g)
    last = 2 * (glen - ref_len)
    ids = [0, 1, 2 * 300, 2 * 300 + 1, 2 * 380, 2 * 390 + 1, 2 * 401, last, last + 1, last + 2, last + 3, 2 ** 40 + 1]
    t = GenomeTable(g, ref_len)
    pq = np.arange(len(ids))
    for lens in ([152, 5, 64, 3], [193, 255, 256, 1]):  # the 3- and the 4-columns-per-lane build
        queries = []
        for x, w in enumerate(ids):
            wb = R.window_bytes(g, ref_len, w)
            queries.append(_mutated_query(rng, wb, lens[x % 4]) if wb else b"<" + _rand(rng, 150) + b">")
        lin = sw_align_arrays(t, ids, pq, queries)
        aff = sw_align_affine_arrays(t, ids, pq, queries, LINEAR)
        _same(aff, lin)
        assert [int(s) for s in aff[0]["status"][-3:]] == [1, 1, 1]  # windows past the genome end
        assert int(aff[0]["status"][4]) == 0
    t.free()


# ------------------------------------------------------------------------------------------ 2. the restatement as oracle
@pytest.mark.parametrize("scoring", SCORINGS)
def test_every_pair_over_two_letters_up_to_length_4(scoring):
    """All 30 x 30 pairs of non-empty strings over {A, C} of length <= 4: every tie shape."""
    from deepreadmapper_amd import sw_align_affine_arrays
    strings = [bytes(b"AC"[(x >> b) & 1] for b in range(n)) for n in range(1, 5) for x in range(1 << n)]
    assert len(strings) == 30
    checked = 0
    for n in range(1, 5):
        windows = [s for s in strings if len(s) == n]
        wid = np.repeat(np.arange(len(windows)), 30)
        pq = np.tile(np.arange(30), len(windows))
        t = _table(windows)
        rec, ops = sw_align_affine_arrays(t, wid, pq, strings, scoring)
        t.free()
        for p in range(len(wid)):
            _check(rec, ops, p, windows[int(wid[p])], strings[int(pq[p])], scoring)
        checked += len(wid)
    assert checked == 900


@pytest.mark.parametrize("scoring", SCORINGS)
def test_random_pairs_up_to_length_40(scoring):
    from deepreadmapper_amd import sw_align_affine_arrays
    rng = np.random.default_rng(90)
    for ref_len in (5, 13, 24, 33, 40):
        for letters in (list(b"AC"), ACGT):
            windows = [_rand(rng, ref_len, letters) for _ in range(30)]
            queries = [_rand(rng, int(rng.integers(1, 41)), letters) for _ in range(30)]
            t = _table(windows)
            rec, ops = sw_align_affine_arrays(t, np.arange(30), np.arange(30), queries, scoring)
            t.free()
            for p in range(30):
                _check(rec, ops, p, windows[p], queries[p], scoring)


def _edited_reads(rng, g, ref_len, columns):
    """(window start, tagged read) pairs: reads of ref_len bases drawn from genome g at a window start, each carrying one
    edit. `columns` are the 1-based query columns (the "<" tag is column 1) on which an indel's first or last base is
    placed: where E crosses from one lane's column group to the next."""
    out = []

    def window_start():
        return int(rng.integers(40, len(g) - ref_len - 40))

    def with_deletion(at, n):  # the read lacks n genome bases after its first `at` bases
        s = window_start()
        return s, g[s:s + at] + g[s + at + n:s + ref_len + n]

    def with_insertion(at, n):  # n foreign bases after the read's first `at` bases
        s = window_start()
        return s, g[s:s + at] + _rand(rng, n) + g[s + at:s + ref_len - n]
    s = window_start()
    sub = bytearray(g[s:s + ref_len])
    sub[ref_len // 2] = ord("A") if sub[ref_len // 2] != ord("A") else ord("C")
    out.append((s, bytes(sub)))
    for n in (1, 2, 5, 20):
        out.append(with_deletion(ref_len // 2 - 3, n))
        out.append(with_insertion(ref_len // 2 + 2, n))
    s = window_start()  # an insertion directly followed by a deletion
    out.append((s, g[s:s + 60] + _rand(rng, 3) + g[s + 64:s + ref_len + 1]))
    for col in columns:
        base = col - 2  # read bases before query column col
        if base + 3 >= ref_len:
            continue
        out.append(with_insertion(base, 2))      # the insertion's first base on column col
        if base >= 1:
            out.append(with_insertion(base - 1, 2))  # ... its last base on column col
        out.append(with_deletion(base, 3))       # a deletion between columns col - 1 and col
    return [(s, b"<" + r + b">") for s, r in out]


def _homopolymer_case(rng, ref_len):
    """A window with a run of 9 A's and reads with one A fewer and one A more: the gap can sit anywhere in the run."""
    w = bytearray(_rand(rng, ref_len))
    w[70:79] = b"A" * 9
    w[69], w[79] = ord("C"), ord("G")
    w = bytes(w)
    fewer = w[:74] + w[75:] + b"T"
    more = w[:74] + b"A" + w[74:-1]
    return w, [b"<" + fewer + b">", b"<" + more + b">"]


@pytest.mark.parametrize("scoring", SCORINGS)
@pytest.mark.parametrize("ref_len", [150, 252])
def test_reads_with_one_edit(ref_len, scoring):
    """150-byte windows against 152-byte reads (3 columns per lane) and 252-byte windows against 254-byte reads (4 per
    lane, the build whose column groups end on 188 to 193): substitution, indels of 1 to 20 bases, an insertion
    followed by a deletion, an indel in a homopolymer, and indels on the lanes' column-group boundaries."""
    from deepreadmapper_amd import sw_align_affine_arrays
    rng = np.random.default_rng(1000 + ref_len)
    g = _rand(rng, 3000)
    columns = [2, 3, 4, 5, 63, 64, 65, 127, 128, 129] + ([188, 189, 190, 191, 192, 193] if ref_len > 190 else [])
    cases = _edited_reads(rng, g, ref_len, columns)
    hw, hq = _homopolymer_case(rng, ref_len)
    windows = [g[s:s + ref_len] for s, _ in cases] + [hw, hw]
    queries = [q for _, q in cases] + hq
    assert {len(q) for q in queries} == {ref_len + 2}
    t = _table(windows)
    rec, ops = sw_align_affine_arrays(t, np.arange(len(windows)), np.arange(len(windows)), queries, scoring)
    t.free()
    for p in range(len(windows)):
        _check(rec, ops, p, windows[p], queries[p], scoring)
    seen = {int(x) & 15 for o in ops for x in o}
    assert seen == {R.M, R.I, R.D}


# ------------------------------------------------------------------------------------------ 3. more pairs than waves
def _grid_waves():
    import ctypes as C
    from deepreadmapper_amd._native import lib

    class Props(C.Structure):
        _fields_ = [("cu_count", C.c_int32), ("clock_khz", C.c_int32), ("total_mem", C.c_int64),
                    ("lds_per_cu", C.c_int32), ("arch", C.c_char * 64)]
    p = Props()
    assert lib().drm_device_get_props(0, C.byref(p)) == 0
    return 16 * p.cu_count  # launch_sw_align_affine's grid bound for a region this short


def test_more_pairs_than_launched_waves():
    """16 windows x 8 queries of 8 bytes, each combination at many batch positions: a wave loops over pairs and reuses
    its LDS."""
    from deepreadmapper_amd import sw_align_affine_arrays
    rng = np.random.default_rng(5)
    scoring = (1, 1, 1, 1)
    windows = [_rand(rng, 8, list(b"AC") if i % 2 else ACGT) for i in range(16)]
    queries = [_rand(rng, 8, list(b"AC") if i % 2 else ACGT) for i in range(8)]
    want = {(w, q): A.align(windows[w], queries[q], scoring) for w in range(16) for q in range(8)}
    npairs = max(5000, _grid_waves() + 37)
    combo = (37 * np.arange(npairs)) % 128
    wid, pq = combo // 8, combo % 8
    t = _table(windows)
    rec, ops = sw_align_affine_arrays(t, wid, pq, queries, scoring)
    t.free()
    assert len(rec) == npairs
    for p in range(npairs):
        r, o = want[(int(wid[p]), int(pq[p]))]
        assert {f: int(rec[f][p]) for f in R.FIELDS} == r, p
        assert [int(x) for x in ops[p]] == o, p


# ------------------------------------------------------------------------------------------ 4. the flank
FLANK_SCORING = (1, 4, 6, 1)


@pytest.fixture(scope="module")
def flank_genome():
    return _rand(np.random.default_rng(2024), 2000)


def _align_region(t, g, wid, q, flank):
    """One pair on genome table t: (record, ops, pos1, cigar), checked against the restatement on the region's bytes
    and against drm_sw_align_region."""
    from deepreadmapper_amd import sam_cigar_region, sw_align_affine_arrays, sw_align_region
    rec, ops = sw_align_affine_arrays(t, [wid], [0], [q], FLANK_SCORING, flank=flank)
    start, n, rev = sw_align_region(t, wid, flank)
    assert (start, n, rev) == A.region(g, 150, wid, flank)
    _check(rec, ops, 0, A.region_bytes(g, 150, wid, flank), q, FLANK_SCORING)
    if int(rec["status"][0]) == 1:
        return rec[0], ops[0], 0, "*"
    pos1, cigar = sam_cigar_region(rec[0], ops[0], len(q), start, n, rev)
    assert (pos1, cigar) == A.sam_fields_region(rec[0], ops[0], len(q), start, n, rev)
    return rec[0], ops[0], pos1, cigar


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("d", [1, 2, 3])
def test_flank_removes_the_window_grid_clip(flank_genome, d, strand):
    """An error-free read that starts d bases after its window's start."""
    from deepreadmapper_amd import GenomeTable
    g = flank_genome
    pos = 700
    read = g[pos + d:pos + d + 150]
    q = b"<" + (R.revcomp(read) if strand else read) + b">"
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    _, _, pos1, cigar = _align_region(t, g, 2 * pos + strand, q, 0)
    assert (pos1, cigar) == (pos + d + 1, f"{150 - d}M{d}S")  # the read's last d bases lie past the window
    rec, _, pos1, cigar = _align_region(t, g, 2 * pos + strand, q, 8)
    t.free()
    assert (pos1, cigar) == (pos + d + 1, "150M") and int(rec["score"]) == 150 and int(rec["nm"]) == 0


@pytest.mark.parametrize("strand", [0, 1])
def test_flank_gives_a_deletion_its_reference_bases(flank_genome, strand):
    """A read that lacks 5 genome bases needs 155 of them; it starts 1 base after the window's start."""
    from deepreadmapper_amd import GenomeTable
    g = flank_genome
    pos = 900
    read = g[pos + 1:pos + 73] + g[pos + 78:pos + 156]
    assert len(read) == 150
    q = b"<" + (R.revcomp(read) if strand else read) + b">"
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    _, _, pos1, cigar = _align_region(t, g, 2 * pos + strand, q, 0)
    m = re.fullmatch(r"(\d+)M5D(\d+)M6S", cigar)
    assert m and int(m.group(1)) + int(m.group(2)) == 144 and pos1 == pos + 2, cigar
    rec, _, pos1, cigar = _align_region(t, g, 2 * pos + strand, q, 8)
    t.free()
    m = re.fullmatch(r"(\d+)M5D(\d+)M", cigar)
    assert m and int(m.group(1)) + int(m.group(2)) == 150 and pos1 == pos + 2, cigar
    assert int(rec["score"]) == 150 - (6 + 5 * 1) and int(rec["nm"]) == 5


def test_flank_is_clamped_at_the_genome_ends(flank_genome):
    from deepreadmapper_amd import GenomeTable, sw_align_region
    g = flank_genome
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    last = len(g) - 150
    for wid, want in ((0, (0, 158, 0)), (1, (0, 158, 1)), (2 * last, (last - 8, 158, 0)), (2 * last + 1, (last - 8, 158, 1)),
                      (2 * 3, (0, 161, 0)), (2 * (last + 1), (0, 0, 0)), (2 * (last + 1) + 1, (0, 0, 1))):
        assert sw_align_region(t, wid, 8) == want
        pos = min(wid // 2, last)
        read = g[pos:pos + 150]
        q = b"<" + (R.revcomp(read) if wid % 2 else read) + b">"
        rec, _, pos1, cigar = _align_region(t, g, wid, q, 8)
        if want[1]:
            assert (pos1, cigar) == (pos + 1, "150M")
        else:
            assert int(rec["status"]) == 1
    t.free()


@pytest.mark.parametrize("flank", [0, 8, 53])  # 150 + 2 * 53 = 256 rows: the cap itself
def test_host_and_device_cut_one_region(flank):
    """drm_sw_align_region, the affine kernel, the MD kernel and (at flank 0) the linear kernel cut the same bytes: the
    read is the region as the host entry gives it, so every kernel must see a full-length exact match of it. Windows
    on both strands that the flank clamps at either genome end by all, one and none of its bases, and one it does not
    clamp."""
    from deepreadmapper_amd import GenomeTable, sw_align_affine_arrays, sw_align_arrays, sw_align_md_arrays, sw_align_region
    ref_len, glen = 150, 600
    g = _rand(np.random.default_rng(600), glen)
    last = glen - ref_len
    # 200 lies 53 bases from both ends: the one region of 256 rows; the last two positions hold no window
    positions = [0, 7, 8, 200, last - 8, last - 7, last, last + 1, 2 ** 40]
    ids = [2 * pos + strand for pos in positions for strand in (0, 1)]
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), ref_len)
    regions = [sw_align_region(t, w, flank) for w in ids]
    for w, got in zip(ids, regions):  # the closed form
        pos, start = w // 2, max(0, w // 2 - flank)
        want = (start, min(glen, pos + ref_len + flank) - start, w % 2) if pos <= last else (0, 0, w % 2)
        assert got == want, (w, flank)
    reads = [(R.revcomp(g[s:s + n]) if rev else g[s:s + n]) if n else g[:ref_len] for s, n, rev in regions]
    pq = np.arange(len(ids))
    rec, ops = sw_align_affine_arrays(t, ids, pq, reads, FLANK_SCORING, flank=flank)
    md, _ = sw_align_md_arrays(t, ids, pq, reads, rec, ops, flank=flank)
    results = [(rec, md)]
    if flank == 0:
        lin = sw_align_arrays(t, ids, pq, reads)
        aff = sw_align_affine_arrays(t, ids, pq, reads, LINEAR)
        _same(aff, lin)
        results.append((lin[0], sw_align_md_arrays(t, ids, pq, reads, *lin)[0]))
    t.free()
    for rec, md in results:
        for p, (_, n, _) in enumerate(regions):
            got = {f: int(rec[f][p]) for f in R.FIELDS}
            if n == 0:
                assert got["status"] == 1 and int(md["status"][p]) == 1, (p, flank)
                continue
            assert got == dict(score=n, ref_begin=0, ref_end=n, q_begin=0, q_end=n, nm=0, n_ops=1, status=0), (p, flank)
            assert (int(md["n_match"][p]), int(md["n_mismatch"][p]), int(md["status"][p])) == (n, 0, 0), (p, flank)
    assert [n for _, n, _ in regions[-4:]] == [0] * 4 and all(n > 0 for _, n, _ in regions[:-4])
    assert flank != 53 or max(n for _, n, _ in regions) == 256


def test_one_row_past_the_cap_is_refused_by_every_entry():
    from deepreadmapper_amd import (DrmError, GenomeTable, sw_align_affine_arrays, sw_align_md_arrays,
                                    sw_align_region)
    from deepreadmapper_amd._native import DRM_ERR_UNSUPPORTED
    g = _rand(np.random.default_rng(600), 600)
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    rec, ops = sw_align_affine_arrays(t, [200], [0], [g[100:250]], FLANK_SCORING)
    for call in (lambda: sw_align_affine_arrays(t, [200], [0], [g[100:250]], FLANK_SCORING, flank=54),
                 lambda: sw_align_md_arrays(t, [200], [0], [g[100:250]], rec, ops, flank=54),
                 lambda: sw_align_region(t, 200, 54)):  # 150 + 2 * 54 = 258 rows
        with pytest.raises(DrmError) as e:
            call()
        assert e.value.code == DRM_ERR_UNSUPPORTED
    t.free()


def test_argument_errors_leave_the_handle_usable(flank_genome):
    from deepreadmapper_amd import DrmError, GenomeTable, sw_align_affine_arrays
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED
    g = flank_genome
    w = g[100:250]
    q = b"<" + w + b">"
    table, genome = _table([w]), GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)

    def code(t, scoring, flank):
        with pytest.raises(DrmError) as e:
            sw_align_affine_arrays(t, [0], [0], [q], scoring, flank=flank)
        return e.value.code
    assert code(table, FLANK_SCORING, 1) == DRM_ERR_ARG  # a window table holds nothing beside its rows
    for t in (table, genome):
        assert code(t, FLANK_SCORING, -1) == DRM_ERR_ARG
        for field, values in enumerate([(0, 32, -1), (0, 64, -1), (-1, 64), (0, 64, -1)]):
            for v in values:
                bad = list(FLANK_SCORING)
                bad[field] = v
                assert code(t, bad, 0) == DRM_ERR_ARG, (field, v)
    assert code(genome, FLANK_SCORING, 54) == DRM_ERR_UNSUPPORTED  # 150 + 2 * 54 = 258 rows
    with pytest.raises(DrmError) as e:
        sw_align_affine_arrays(genome, [0], [0], [b"A" * 257], FLANK_SCORING)
    assert e.value.code == DRM_ERR_UNSUPPORTED
    for t, wid, flank in ((table, 0, 0), (genome, 200, 53)):  # 150 + 2 * 53 = 256 rows is the limit itself
        rec, ops = sw_align_affine_arrays(t, [wid], [0], [q], (31, 63, 63, 63), flank=flank)
        assert (int(rec["score"][0]), R.cigar_string(ops[0])) == (31 * 150, "150M")
        t.free()


# ------------------------------------------------------------------------------------------ 5. device entry point
def test_device_entry_point_equals_host(flank_genome):
    from deepreadmapper_amd import GenomeTable, sw_align_affine_arrays
    from deepreadmapper_amd import rerank as RR
    from deepreadmapper_amd._native import check, lib
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    g = flank_genome
    rng = np.random.default_rng(17)
    n = 300
    wid = rng.integers(0, 2 * (len(g) - 150) + 6, size=n).astype(np.uint64)  # a few past the genome end
    queries = [_mutated_query(rng, R.window_bytes(g, 150, int(w) % (2 * (len(g) - 150))), 152) for w in wid[:24]]
    pq = (np.arange(n) % 24).astype(np.int64)
    wid[:24] = wid[:24] % (2 * (len(g) - 150))
    wid[30] = 2 * (len(g) - 150) + 2  # a window past the genome end
    pq[7] = 24   # the device form cannot refuse a query index outside [0, nq): such a pair is status 1
    pq[11] = -1
    qbuf, qlen = RR.pack_queries(queries)
    sc = RR.sw_scoring((2, 4, 4, 2))
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    st = Stream()
    d = [DeviceBuffer.from_host(x) for x in (wid, pq, qbuf, qlen)]
    d_rec, d_ops = DeviceBuffer(n, RR.SW_ALIGNMENT_DTYPE), DeviceBuffer((n, 16), np.uint32)
    d_ops.zero()
    check(lib().drm_sw_align_affine_device(t.handle, sc.ctypes.data, 8, d[0].ptr, d[1].ptr, n, d[2].ptr, d[3].ptr,
                                           qbuf.shape[1], len(qlen), d_rec.ptr, d_ops.ptr, 16, st.handle))
    st.synchronize()
    rec, ops = d_rec.download(), d_ops.download()
    ok = np.ones(n, bool)
    ok[[7, 11]] = False
    want, wops = sw_align_affine_arrays(t, wid[ok], pq[ok], queries, (2, 4, 4, 2), flank=8)
    t.free()
    assert rec[ok].tobytes() == want.tobytes()
    assert (want["status"][:20] == 0).all() and (want["status"] == 1).any()
    assert [list(map(int, ops[p, :rec["n_ops"][p]])) for p in np.flatnonzero(ok)] == [list(map(int, o)) for o in wops]
    assert [tuple(int(x) for x in r) for r in rec[~ok]] == [(0, 0, 0, 0, 0, 0, 0, 1)] * 2


# ------------------------------------------------------------------------------------------ 6. CLI
def test_pipeline_cli_sam_scoring_and_flank(tmp_path):
    """test_gpu_sw_align.py's streaming SAM recipe with DRM_SAM_SCORING=1,4,6,1 DRM_SAM_FLANK=8: every line is the one
    composed from sw_align_affine_arrays + sam_cigar_region."""
    from deepreadmapper_amd import (GenomeTable, extract_fasta_sequence, sam_cigar_region, sw_align_affine_arrays,
                                    sw_align_region)
    fna = os.path.join(GOLDEN, "ecoli_150.fna")
    fq = os.path.join(GOLDEN, "test_data.fastq")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    for v in ("DRM_SAM_CIGAR", "DRM_SAM_SCORING", "DRM_SAM_FLANK"):
        env.pop(v, None)
    r = subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), fna, "c1", "150"], cwd=tmp_path, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    base = [os.path.join(ROOT, "bin", "pipeline"), "c1", fq, fna, "128", "4", "4"]

    def run(name, extra, **more):
        return subprocess.run(base + [name] + extra, cwd=tmp_path, env=dict(env, DRM_SAM_BLOCK="40", **more),
                              capture_output=True, text=True)
    r = run("static", ["0", "0"])
    assert r.returncode == 0, r.stdout + r.stderr
    g = extract_fasta_sequence(fna)
    lines = open(fq, "rb").read().split(b"\n")
    recs = [(lines[i], lines[i + 1]) for i in range(0, len(lines) - 1, 4) if lines[i].startswith(b"@")]
    qids = [h[1:].split(b" ")[0].split(b"\t")[0].split(b"/")[0].decode() for h, _ in recs]
    ids = np.load(tmp_path / "static" / "indices.npy")
    assert ids.shape == (len(recs), 4)
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    queries = [b"<" + read + b">" for _, read in recs]

    def composed(scoring, flank):
        rec, ops = sw_align_affine_arrays(t, ids.reshape(-1), np.repeat(np.arange(len(recs)), 4), queries, scoring,
                                          flank=flank)
        want = ["@HD\tVN:1.0\tSO:unsorted", "@SQ\tSN:ref\tLN:150"]
        mapped = 0
        for i, (_, read) in enumerate(recs):
            for j in range(4):
                p, wid = 4 * i + j, int(ids[i, j])
                flag = (0 if j == 0 else 256) | (16 if wid % 2 else 0)
                seq = (R.revcomp(read) if wid % 2 else read).decode()
                if int(rec["status"][p]) == 1:
                    want.append(f"{qids[i]}\t{flag | 4}\tref\t0\t60\t*\t*\t0\t0\t{seq}\t*")
                    continue
                start, n, rev = sw_align_region(t, wid, flank)
                pos1, cigar = sam_cigar_region(rec[p], ops[p], len(read) + 2, start, n, rev)
                assert R.cigar_query_length(cigar) == len(seq)
                want.append(f"{qids[i]}\t{flag}\tref\t{pos1}\t60\t{cigar}\t*\t0\t0\t{seq}\t*"
                            f"\tAS:i:{int(rec['score'][p])}\tNM:i:{int(rec['nm'][p])}")
                mapped += 1
        assert mapped > len(recs)
        return want
    # a flank alone means the scoring 1,1,0,1
    for name, more, scoring in (("affine", {"DRM_SAM_SCORING": "1,4,6,1", "DRM_SAM_FLANK": "8"}, (1, 4, 6, 1)),
                                ("flank", {"DRM_SAM_FLANK": "8"}, LINEAR)):
        r = run(name, ["1", "1"], DRM_SAM_CIGAR="1", **more)
        assert r.returncode == 0, r.stdout + r.stderr
        got = open(tmp_path / name / "results.sam").read().split("\n")
        assert got[-1] == "" and got[:-1] == composed(scoring, 8), name
    t.free()
    # a malformed value ends the run before any work
    for bad in ({"DRM_SAM_SCORING": "1,4,6"}, {"DRM_SAM_SCORING": "1,4,x,1"}, {"DRM_SAM_SCORING": "0,4,6,1"},
                {"DRM_SAM_FLANK": "-1"}, {"DRM_SAM_FLANK": "54"}):
        r = run("bad", ["1", "1"], DRM_SAM_CIGAR="1", **bad)
        assert r.returncode == 1 and r.stderr.startswith("Error:"), (bad, r.stdout, r.stderr)
        assert "Index loaded" not in r.stdout and not os.path.exists(tmp_path / "bad" / "results.sam")
    # without DRM_SAM_CIGAR=1 neither variable has any effect
    r = run("plain", ["1", "1"])
    assert r.returncode == 0, r.stdout + r.stderr
    r = run("ignored", ["1", "1"], DRM_SAM_SCORING="1,4,6,1", DRM_SAM_FLANK="8")
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "ignored" / "results.sam", "rb").read() == open(tmp_path / "plain" / "results.sam", "rb").read()
    r = run("ignored2", ["1", "1"], DRM_SAM_SCORING="garbage")
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "ignored2" / "results.sam", "rb").read() == open(tmp_path / "plain" / "results.sam", "rb").read()
