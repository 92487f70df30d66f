"""GPU tests of the end-aware affine-gap alignment (sw_align_affine.hip's end-aware instantiation,
drm_sw_align_affine_clip): record and words equal the Python restatement of the definition
(tests/sw_align_clip_ref.py) on every small pair and on the shapes where the per-column floor and the end column meet
the lanes' column groups; at penalty 0 it is drm_sw_align_affine byte for byte; the device form equals the host form;
the statuses; and its records feed the MD pass."""
import functools

import numpy as np
import pytest

import md_ref as MD
import sw_align_affine_ref as A
import sw_align_clip_ref as K
import sw_align_ref as R

pytestmark = pytest.mark.gpu

ACGT = list(b"ACGT")
SCORINGS = [(1, 4, 6, 1), (2, 4, 4, 2), (1, 1, 1, 1), (1, 3, 5, 2)]  # test_gpu_sw_align_affine.py's
TAGS = [(0, 0), (1, 1), (3, 2), (4, 0), (0, 4)]
SHORT_LENS = [3, 4, 63, 64, 65, 150, 151, 152, 191, 192]  # the 3-columns-per-lane build
LONG_LENS = [193, 253, 254, 255, 256]                     # the 4-columns-per-lane build


def _rand(rng, n, letters=ACGT):
    return bytes(rng.choice(letters, size=n).astype(np.uint8))


def _table(windows):
    from deepreadmapper_amd import WindowTable
    return WindowTable(np.frombuffer(b"".join(windows), dtype=np.uint8).reshape(len(windows), len(windows[0])))


def _check(rec, ops, p, w, q, scoring, L, tags):
    """Pair p of a wrapper result equals the restatement on (w, q), and its operations replay to its score."""
    want, wops = K.align(w, q, scoring, L, tags)
    got = {f: int(rec[f][p]) for f in R.FIELDS}
    assert got == want, (p, w, q, scoring, L, tags, got, want)
    assert [int(x) for x in ops[p]] == wops, (p, w, q, scoring, L, tags)
    if want["status"] == 0:
        assert A.replay(w, q, rec[p], ops[p], scoring) == (got["score"], got["nm"]), (p, w, q, scoring, L, tags)
    return want


def _flip(base):
    return ord("A") if base != ord("A") else ord("C")


def _end_edited(rng, orig, core, variant):
    """A read of exactly `core` bases from orig (core + 1 bases): substitutions in its first and last three columns,
    or an indel within five bases of an end, by `variant`."""
    s = bytearray(orig[:core])
    if core < 8:
        if core and variant % 2:
            s[int(rng.integers(core))] = int(rng.choice(ACGT))
        return bytes(s)
    v = variant % 10
    if v < 3:
        s[v] = _flip(s[v])                      # read column 0, 1 or 2
    elif v < 6:
        s[core - 1 - (v - 3)] = _flip(s[core - 1 - (v - 3)])  # the last, the one before, the third from the end
    elif v == 6:
        s[0], s[core - 1] = _flip(s[0]), _flip(s[core - 1])
    elif v == 7:
        s = bytearray(orig[:4] + orig[5:core + 1])  # a deletion after the read's first 4 bases
    elif v == 8:
        s = bytearray(orig[:core - 4] + _rand(rng, 1) + orig[core - 4:core - 1])  # an insertion 3 bases from its end
    else:
        s = bytearray(orig[:core - 5] + orig[core - 4:core + 1])  # a deletion 4 bases from its end
    assert len(s) == core
    return bytes(s)


def _wrap(read, tags):
    return b"<" * tags[0] + read + b">" * tags[1]


# ------------------------------------------------------------------------------------------ 1. exhaustive small pairs
@pytest.mark.parametrize("scoring", SCORINGS)
def test_every_pair_over_two_letters_up_to_length_4(scoring):
    """All 30 x 30 pairs of non-empty strings over {A, C} of length <= 4, bare with tags (0, 0) and wrapped in "<" ">"
    with tags (1, 1), under four penalties: every tie shape at the two floors."""
    from deepreadmapper_amd import sw_align_affine_clip_arrays
    strings = [bytes(b"AC"[(x >> b) & 1] for b in range(n)) for n in range(1, 5) for x in range(1 << n)]
    assert len(strings) == 30
    checked, changed = 0, 0
    for n in range(1, 5):
        windows = [s for s in strings if len(s) == n]
        wid = np.repeat(np.arange(len(windows)), 30)
        pq = np.tile(np.arange(30), len(windows))
        t = _table(windows)
        for tags in ((0, 0), (1, 1)):
            queries = [_wrap(s, tags) for s in strings]
            for L in (0, 1, 2, 5):
                rec, ops = sw_align_affine_clip_arrays(t, wid, pq, queries, scoring, L, tags=tags)
                for p in range(len(wid)):
                    w, q = windows[int(wid[p])], queries[int(pq[p])]
                    want = _check(rec, ops, p, w, q, scoring, L, tags)
                    changed += L > 0 and want != A.align(w, q, scoring)[0]
                checked += len(wid)
        t.free()
    assert checked == 900 * 2 * 4 and changed > 100


# ------------------------------------------------------------------------------------------ 2. lane boundaries
LANE_SCORING = (1, 4, 6, 1)


@functools.lru_cache(maxsize=None)
def _table_cases(ref_len, short):
    """(windows, queries, tags per pair) for one table: a row per pair, every query length of one build under every
    tag pair, the read drawn from its row with an edit at an end."""
    rng = np.random.default_rng(300 + 2 * ref_len + short)
    windows, queries, tags_of = [], [], []
    for x, q_len in enumerate(SHORT_LENS if short else LONG_LENS):
        for y, tags in enumerate(TAGS):
            core = q_len - sum(tags)
            if core < 0:  # no read between the tags: b < a
                windows.append(_rand(rng, ref_len))
                queries.append((b"<" * tags[0] + b">" * tags[1])[:q_len])
                tags_of.append(tags)
                continue
            orig = _rand(rng, core + 1)
            if core + 1 <= ref_len:
                at = int(rng.integers(ref_len - core))
                row = _rand(rng, at) + orig + _rand(rng, ref_len - core - 1 - at)
            else:
                at = int(rng.integers(core + 2 - ref_len))
                row = orig[at:at + ref_len]
            assert len(row) == ref_len
            windows.append(row)
            queries.append(_wrap(_end_edited(rng, orig, core, x + 3 * y), tags))
            tags_of.append(tags)
            assert len(queries[-1]) == q_len
    return windows, queries, tags_of


@pytest.mark.parametrize("L", [5, 63])
@pytest.mark.parametrize("ref_len", [1, 3, 150, 256])
def test_query_lengths_and_tags_on_the_lanes_column_groups(ref_len, L):
    """b = q_len - tag_postfix on every column residue of a lane in both builds, a = tag_prefix on a lane's last
    column (3 in the 3-column build, 4 in the 4-column one) and on the next lane's first."""
    from deepreadmapper_amd import sw_align_affine_clip_arrays
    mapped = clipped_less = 0
    for short in (True, False):
        windows, queries, tags_of = _table_cases(ref_len, short)
        t = _table(windows)
        for tags in TAGS:
            sel = [p for p in range(len(windows)) if tags_of[p] == tags]
            rec, ops = sw_align_affine_clip_arrays(t, sel, sel, queries, LANE_SCORING, L, tags=tags)
            for x, p in enumerate(sel):
                want = _check(rec, ops, x, windows[p], queries[p], LANE_SCORING, L, tags)
                mapped += want["status"] == 0
                local = A.align(windows[p], queries[p], LANE_SCORING)[0]
                clipped_less += want["status"] == 0 and \
                    want["q_end"] - want["q_begin"] > local["q_end"] - local["q_begin"]
        t.free()
    if ref_len >= 150:
        assert mapped >= 55 and clipped_less >= 10


@functools.lru_cache(maxsize=None)
def _genome_cases():
    rng = np.random.default_rng(77)
    g = _rand(rng, 1200)
    last = len(g) - 150
    ids = [0, 1, 2 * 3, 2 * 3 + 1, 2 * 500, 2 * 500 + 1, 2 * 640 + 1, 2 * last, 2 * last + 1, 2 * (last - 2),
           2 * (last - 2) + 1, 2 * (last + 1), 2 * (last + 1) + 1]
    wid, queries = [], []
    for x, w in enumerate(ids):
        for v in range(10):
            wb = R.window_bytes(g, 150, w)
            # the read starts a base or two off the window grid, so that a flank has something to add
            # (151 bases, the last being the one that follows the read on its own strand)
            if w % 2:
                pos = min(max(w // 2 + (v % 3) - 1, 1), last)
                orig = R.revcomp(g[pos - 1:pos + 150])
            else:
                pos = min(max(w // 2 + (v % 3) - 1, 0), last - 1)
                orig = g[pos:pos + 151]
            wid.append(w)
            queries.append(_wrap(_end_edited(rng, orig, 150, v + x) if wb else _rand(rng, 150), (1, 1)))
    return g, wid, queries


@pytest.mark.parametrize("flank", [0, 8, 53])
def test_genome_regions_both_strands_and_clamped_flanks(flank):
    """ref_len 150 on a genome handle: flank 53 makes the region 256 rows; windows at genome position 0 and at the
    genome's end, where the flank is clamped; a window past the end is status 1."""
    from deepreadmapper_amd import GenomeTable, sw_align_affine_clip_arrays
    g, wid, queries = _genome_cases()
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    pq = np.arange(len(wid))
    full = 0
    for L in (5, 17):
        rec, ops = sw_align_affine_clip_arrays(t, wid, pq, queries, LANE_SCORING, L, flank=flank)
        for p in range(len(wid)):
            want = _check(rec, ops, p, A.region_bytes(g, 150, wid[p], flank), queries[p], LANE_SCORING, L, (1, 1))
            full += want["status"] == 0 and (want["q_begin"], want["q_end"]) == (1, 151)
        assert [int(s) for s in rec["status"][-20:]] == [1] * 20  # the two windows past the genome end
        assert (rec["status"][:-20] == 0).all()
    assert full > 50
    if flank == 53:  # the 4-column build over 256 rows: 254-base reads from the region itself, (3, 2) tags included
        rng = np.random.default_rng(78)
        ids = [2 * 500, 2 * 500 + 1, 2 * 300 + 1, 2 * 700]
        for tags, core in (((1, 1), 254), ((3, 2), 251), ((4, 0), 252), ((0, 4), 249)):
            qs = []
            for v, w in enumerate(ids):
                region = A.region_bytes(g, 150, w, 53)
                assert len(region) == 256
                qs.append(_wrap(_end_edited(rng, region[1:core + 2], core, 3 * v + core), tags))
            rec, ops = sw_align_affine_clip_arrays(t, ids, np.arange(4), qs, LANE_SCORING, 5, tags=tags, flank=53)
            for p, w in enumerate(ids):
                _check(rec, ops, p, A.region_bytes(g, 150, w, 53), qs[p], LANE_SCORING, 5, tags)
    t.free()


# ------------------------------------------------------------------------------------------ 3. penalty 0
@pytest.mark.parametrize("ref_len", [3, 150, 256])
def test_penalty_0_equals_the_affine_kernel_on_a_table(ref_len):
    from deepreadmapper_amd import sw_align_affine_arrays, sw_align_affine_clip_arrays
    for short in (True, False):
        windows, queries, _ = _table_cases(ref_len, short)
        ids = list(range(len(windows))) + [len(windows)]  # the last lies outside the table
        pq = list(range(len(windows))) + [0]
        t = _table(windows)
        for scoring in (LANE_SCORING, (1, 1, 0, 1)):
            plain = sw_align_affine_arrays(t, ids, pq, queries, scoring)
            assert (plain[0]["status"] == 0).sum() >= len(windows) // 2
            for tags in ((0, 0), (1, 1), (4, 0)):
                got = sw_align_affine_clip_arrays(t, ids, pq, queries, scoring, 0, tags=tags)
                # a pair whose tags leave no read is status 1 at any penalty
                keep = np.array([len(queries[q]) - tags[1] >= tags[0] for q in pq])
                assert got[0][keep].tobytes() == plain[0][keep].tobytes()
                assert [list(map(int, o)) for o, k in zip(got[1], keep) if k] == \
                    [list(map(int, o)) for o, k in zip(plain[1], keep) if k]
                assert (got[0]["status"][~keep] == 1).all()
        t.free()


def test_penalty_0_equals_the_affine_kernel_on_a_genome():
    from deepreadmapper_amd import GenomeTable, sw_align_affine_arrays, sw_align_affine_clip_arrays
    g, wid, queries = _genome_cases()
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    pq = np.arange(len(wid))
    for flank in (0, 8, 53):
        plain = sw_align_affine_arrays(t, wid, pq, queries, LANE_SCORING, flank=flank)
        got = sw_align_affine_clip_arrays(t, wid, pq, queries, LANE_SCORING, 0, flank=flank)
        assert got[0].tobytes() == plain[0].tobytes()
        assert [list(map(int, o)) for o in got[1]] == [list(map(int, o)) for o in plain[1]]
    t.free()


# ------------------------------------------------------------------------------------------ 4. device form
def _device_call(t, scoring, clip, flank, wid, pq, qbuf, qlen, stride):
    from deepreadmapper_amd import rerank as RR
    from deepreadmapper_amd._native import check, lib
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    n = len(wid)
    sc, cl = RR.sw_scoring(scoring), np.array(clip, dtype=np.int32)
    st = Stream()
    d = [DeviceBuffer.from_host(x) for x in (np.asarray(wid, np.uint64), np.asarray(pq, np.int64), qbuf, qlen)]
    d_rec, d_ops = DeviceBuffer(n, RR.SW_ALIGNMENT_DTYPE), DeviceBuffer((n, stride), np.uint32)
    d_ops.zero()
    check(lib().drm_sw_align_affine_clip_device(t.handle, sc.ctypes.data, cl.ctypes.data, flank, d[0].ptr, d[1].ptr, n,
                                                d[2].ptr, d[3].ptr, qbuf.shape[1], len(qlen), d_rec.ptr, d_ops.ptr,
                                                stride, st.handle))
    st.synchronize()
    return d_rec.download(), d_ops.download()


def test_device_entry_point_equals_host():
    from deepreadmapper_amd import GenomeTable, sw_align_affine_clip_arrays
    from deepreadmapper_amd import rerank as RR
    g, wid, queries = _genome_cases()
    wid, n = np.array(wid, dtype=np.uint64), len(wid)
    pq = np.arange(n, dtype=np.int64)
    pq[7], pq[11] = n, -1  # the device form cannot refuse a query index outside [0, nq): such a pair is status 1
    qbuf, qlen = RR.pack_queries(queries)
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    rec, ops = _device_call(t, (2, 4, 4, 2), (5, 1, 1), 8, wid, pq, qbuf, qlen, 16)
    ok = np.ones(n, bool)
    ok[[7, 11]] = False
    want, wops = sw_align_affine_clip_arrays(t, wid[ok], pq[ok], queries, (2, 4, 4, 2), 5, flank=8)
    t.free()
    assert rec[ok].tobytes() == want.tobytes()
    assert (want["status"] == 0).sum() > 100 and (want["status"] == 1).any()
    assert [list(map(int, ops[p, :rec["n_ops"][p]])) for p in np.flatnonzero(ok)] == [list(map(int, o)) for o in wops]
    assert [tuple(int(x) for x in r) for r in rec[~ok]] == [(0, 0, 0, 0, 0, 0, 0, 1)] * 2


# ------------------------------------------------------------------------------------------ 5. statuses, arguments
def test_statuses():
    from deepreadmapper_amd import GenomeTable, sw_align_affine_clip_arrays
    from deepreadmapper_amd import rerank as RR
    rng = np.random.default_rng(4)
    g = _rand(rng, 600)
    w = g[100:250]
    t, gt = _table([w]), GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    q = b"<<<" + w + b">>"
    none = (0, 0, 0, 0, 0, 0, 0, 1)
    # tags (3, 2): a 4-byte query has b = 2 < a = 3; a 5-byte one holds no read column but is no error
    rec, ops = sw_align_affine_clip_arrays(t, [0, 0, 0, 1, 2 ** 40 + 1], [0, 1, 2, 0, 0], [q, b"<<<>", b"<<<>>"],
                                           LANE_SCORING, 5, tags=(3, 2))
    assert R.cigar_string(ops[0]) == "150M" and int(rec["score"][0]) == 150
    assert [tuple(int(x) for x in r) for r in rec[1:]] == [none] * 4
    past = 2 * (600 - 150) + 2
    rec, ops = sw_align_affine_clip_arrays(gt, [200, past, past + 1], [0, 0, 0], [q], LANE_SCORING, 5, tags=(3, 2),
                                           flank=8)
    assert int(rec["status"][0]) == 0 and [tuple(int(x) for x in r) for r in rec[1:]] == [none] * 2
    # a pair_query outside [0, nq) on the device form
    qbuf, qlen = RR.pack_queries([q])
    rec, _ = _device_call(t, LANE_SCORING, (5, 3, 2), 0, [0, 0, 0], [0, 1, -1], qbuf, qlen, 16)
    assert int(rec["status"][0]) == 0 and [tuple(int(x) for x in r) for r in rec[1:]] == [none] * 2
    # more runs than ops_stride: status 2, the first words stored, n_ops the full count
    read = bytearray(w)
    for at in (20, 50, 80, 110):
        del read[at]
        read.insert(at + 10, ord("A"))
    q2 = b"<" + bytes(read) + b">"
    want, wops = K.align(w, q2, (1, 1, 1, 1), 5)
    assert want["n_ops"] > 4
    qbuf, qlen = RR.pack_queries([q2])
    rec, ops = _device_call(t, (1, 1, 1, 1), (5, 1, 1), 0, [0], [0], qbuf, qlen, 4)
    assert {f: int(rec[f][0]) for f in R.FIELDS} == want | {"status": 2}
    assert [int(x) for x in ops[0]] == wops[:4]
    rec, ops = sw_align_affine_clip_arrays(t, [0], [0], [q2], (1, 1, 1, 1), 5, ops_stride=4)  # the wrapper's retry
    _check(rec, ops, 0, w, q2, (1, 1, 1, 1), 5, (1, 1))
    t.free()
    gt.free()


def test_argument_errors_leave_the_handle_usable():
    from deepreadmapper_amd import DrmError, GenomeTable, sw_align_affine_clip_arrays
    from deepreadmapper_amd._native import DRM_ERR_ARG, DRM_ERR_UNSUPPORTED
    rng = np.random.default_rng(6)
    g = _rand(rng, 600)
    w = g[100:250]
    q = b"<" + w + b">"
    table, genome = _table([w]), GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)

    def code(t, scoring, clip, tags, flank):
        with pytest.raises(DrmError) as e:
            sw_align_affine_clip_arrays(t, [0], [0], [q], scoring, clip, tags=tags, flank=flank)
        return e.value.code
    for t in (table, genome):
        for clip, tags in ((-1, (1, 1)), (64, (1, 1)), (5, (-1, 1)), (5, (1, -1))):
            assert code(t, LANE_SCORING, clip, tags, 0) == DRM_ERR_ARG, (clip, tags)
        assert code(t, (0, 4, 6, 1), 5, (1, 1), 0) == DRM_ERR_ARG
        assert code(t, LANE_SCORING, 5, (1, 1), -1) == DRM_ERR_ARG
    assert code(table, LANE_SCORING, 5, (1, 1), 1) == DRM_ERR_ARG
    assert code(genome, LANE_SCORING, 5, (1, 1), 54) == DRM_ERR_UNSUPPORTED
    for t, wid, flank in ((table, 0, 0), (genome, 200, 53)):
        rec, ops = sw_align_affine_clip_arrays(t, [wid], [0], [q], (31, 63, 63, 63), 63, flank=flank)
        assert (int(rec["score"][0]), R.cigar_string(ops[0])) == (31 * 150, "150M")
        t.free()


# ------------------------------------------------------------------------------------------ 6. the MD pass
@pytest.mark.parametrize("flank", [0, 8])
def test_records_feed_the_md_pass(flank):
    """Every status-0 record is a walk the MD kernel accepts (status 0, never 3), and the read, the CIGAR and the MD
    string rebuild the genome bytes under the alignment."""
    from deepreadmapper_amd import (GenomeTable, sam_cigar_region, sam_md, sw_align_affine_clip_arrays,
                                    sw_align_md_arrays, sw_align_region)
    g, wid, queries = _genome_cases()
    t = GenomeTable(np.frombuffer(g, dtype=np.uint8), 150)
    pq = np.arange(len(wid))
    rebuilt = 0
    for L in (5, 63):
        rec, ops = sw_align_affine_clip_arrays(t, wid, pq, queries, LANE_SCORING, L, flank=flank)
        h, words = sw_align_md_arrays(t, wid, pq, queries, rec, ops, flank=flank)
        for p in range(len(wid)):
            assert int(h["status"][p]) == int(rec["status"][p]) in (0, 1), (p, h[p], rec[p])
            if int(rec["status"][p]):
                continue
            region = A.region_bytes(g, 150, wid[p], flank)
            want, wwords = MD.md_words(region, queries[p], rec[p], ops[p])
            assert {f: int(h[f][p]) for f in MD.MD_FIELDS} == want and [int(x) for x in words[p]] == wwords
            assert want["n_mismatch"] + want["n_ins"] + want["n_del"] == int(rec["nm"][p])
            start, n, rev = sw_align_region(t, wid[p], flank)
            pos1, cigar = sam_cigar_region(rec[p], ops[p], len(queries[p]), start, n, rev)
            read = queries[p][1:-1]
            seq = R.revcomp(read) if rev else read
            ref = MD.rebuild_reference(seq, cigar, sam_md(h[p], words[p], rev))
            assert ref == g[pos1 - 1:pos1 - 1 + len(ref)], (p, cigar)
            rebuilt += 1
    t.free()
    assert rebuilt > 200
