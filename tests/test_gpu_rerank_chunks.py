"""The chunked SW rerank (sw_rerank.hip, `launch_sw_pair_profile`; DESIGN.md sec. 4.4 "Round 8"): a call's queries split
into chunks that alternate between two streams of the window-table handle, each chunk's flagged re-scores and top-k
behind its own scoring, and the re-score kernel running over the list of queries the scoring flagged. Every case is
compared with the oracle's post_process_sw_static (or _dynamic) and, byte for byte, with the same call as one launch
sequence on the caller's stream (`sw_chunk = 0`). The chunk size is forced per handle (`WindowTable.sw_chunk`, the
DRM_SW_CHUNK knob's setter) to 96 queries, which is not a multiple of the top-k kernel's 64-query block.
* chunk and sort-block edges: 1, 95, 96, 97, 192, 193 and 2 * 96 + 3 tagged 152-byte queries, 1, 64, 65 and 128
  candidates each;
* flagged queries (an N against a window holding N) first in a chunk, last in a chunk, a whole chunk, none: the list
  path and the empty list, and the rows equal the bit-profile kernel's own (one child under DRM_SW_BITPROFILE=1);
* 64-byte queries, the dynamic lookup and sparse strides 2 to 4 across a chunk edge; the library's own plan
  (`sw_chunk = -1`) on 140,000 short queries;
* two calls back to back on one stream, one synchronise: the second must not touch the workspace the first call's
  top-k still reads; with the chunk size the same and different between the two;
* several handles made and freed in a row (each owns two streams and three events)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rerank_cases as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu

CHUNK = 96
WIN = 150
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sw_chunk_child.py")


def _check(got, want, k):
    """GPU rows (scores, ids, counts) against the oracle's, up to each query's count"""
    sc, ids, cnt = got
    sc_o, id_o, cnt_o = want
    assert np.array_equal(cnt, cnt_o)
    m = np.arange(k)[None] < cnt[:, None]
    bad = np.flatnonzero(((sc != sc_o) & m).any(axis=1) | ((ids != id_o) & m).any(axis=1))
    assert bad.size == 0, f"{bad.size} queries differ from the oracle, first {bad[:8]}"


def _chunked_and_whole(t, call, chunk=CHUNK):
    """`call()` on handle t in chunks and as one launch sequence: equal bytes; returns the chunked rows"""
    t.sw_chunk = chunk
    assert t.sw_chunk == chunk
    a = call()
    t.sw_chunk = 0
    b = call()
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    return a


def _tagged_reads(rng, refs, nq, cols=150):
    from deepreadmapper_amd.rerank import pack_queries
    reads, own = zip(*[G.dna_read(rng, refs, i, cols, True) for i in range(nq)])
    return pack_queries(reads), np.array(own)


# ------------------------------------------------------------------------------------------ 1. chunk and block edges
NQ_EDGES = [1, 95, 96, 97, 192, 193, 2 * CHUNK + 3]
_edge_cache = {}


def _edge_case(ncand):
    """the largest batch and its oracle rows, once per list length: the smaller batches are its first queries"""
    if ncand not in _edge_cache:
        rng = np.random.default_rng(80_000 + ncand)
        refs = G.windows(rng, WIN)
        (q, ql), own = _tagged_reads(rng, refs, max(NQ_EDGES))
        assert q.shape[1] == 152
        nb = G.lists(rng, own, len(refs), ncand)
        rc, sc, ids, cnt = O.post_process_sw_static(nb, refs, WIN, q, ql, 1, ncand, ncand)
        assert rc == 0
        _edge_cache[ncand] = (refs, nb, q, ql, (sc, ids, cnt))
    return _edge_cache[ncand]


@pytest.mark.parametrize("ncand", [1, 64, 65, 128])
def test_chunk_and_sort_block_edges(ncand):
    """96-query chunks against the top-k's 64-query blocks: a call of one chunk (1, 95, 96: no streams used), a second
    chunk of one query (97), two full chunks (192), a third of one (193) and of three (195); lists of one candidate,
    of one full pass of the wave's first halves (64), one second half (65) and all of them (128)."""
    from deepreadmapper_amd import WindowTable, rerank_arrays
    refs, nb, q, ql, want = _edge_case(ncand)
    t = WindowTable(refs)
    for nq in NQ_EDGES:
        got = _chunked_and_whole(t, lambda: rerank_arrays(t, nb[:nq], (q[:nq], ql[:nq]), 1, ncand, ncand))
        _check(got, tuple(x[:nq] for x in want), ncand)
    t.free()


# ------------------------------------------------------------------------------------------ 2. flagged queries
PLACEMENTS = {"first_of_chunk": [CHUNK], "last_of_chunk": [CHUNK - 1, 3 * CHUNK - 1],
              "whole_chunk": list(range(CHUNK, 2 * CHUNK)), "none": []}
FLAG_NQ, FLAG_NC = 3 * CHUNK, 24


def _flag_batches():
    """per placement: windows 48.. hold an N at column 70; a flagged query is such a window, tagged, with that window
    first in its list; every other query and list stays clear of them"""
    rng = np.random.default_rng(81_000)
    refs = G.windows(rng, WIN, n_dna=64, n_alpha=0)
    refs[48:, 70] = ord("N")
    out = {}
    for name, where in PLACEMENTS.items():
        (q, ql), own = _tagged_reads(rng, refs, FLAG_NQ)  # own windows are 0..47: no N
        nb = rng.integers(0, 48, size=(FLAG_NQ, FLAG_NC)).astype(np.int64)
        nb[:, 0] = own
        for j, i in enumerate(where):
            w = 48 + j % 16
            q[i, 1:151] = refs[w]
            nb[i, 0] = w
        out[name] = (nb, q, ql)
    return refs, out


@pytest.fixture(scope="module")
def flag_cases(tmp_path_factory):
    """the batches, the oracle's rows and the bit-profile kernel's rows (one child process for all placements)"""
    refs, batches = _flag_batches()
    d = tmp_path_factory.mktemp("sw_chunks")
    src, dst = str(d / "in.npz"), str(d / "out.npz")
    arrays = {"refs": refs}
    for i, (nb, q, ql) in enumerate(batches.values()):
        arrays.update({f"nb{i}": nb, f"q{i}": q, f"ql{i}": ql})
    np.savez(src, **arrays)
    argv = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, src, dst]
    r = subprocess.run(argv, env=dict(os.environ, DRM_SW_BITPROFILE="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    bits = np.load(dst)
    want = {}
    for i, (name, (nb, q, ql)) in enumerate(batches.items()):
        rc, sc, ids, cnt = O.post_process_sw_static(nb, refs, WIN, q, ql, 1, FLAG_NC, FLAG_NC)
        assert rc == 0
        _check((bits[f"sc{i}"], bits[f"ids{i}"], bits[f"cnt{i}"]), (sc, ids, cnt), FLAG_NC)
        want[name] = ((sc, ids, cnt), (bits[f"sc{i}"], bits[f"ids{i}"], bits[f"cnt{i}"]))
    return refs, batches, want


@pytest.mark.parametrize("placement", list(PLACEMENTS))
def test_flagged_queries(flag_cases, placement):
    """The scoring kernel lists the queries it flagged per chunk and the re-score kernel strides over that list: a
    flagged query first in its chunk, last in its chunk (and last of the call), a chunk of nothing else, and an empty
    list. A flagged query scores its own window 150 (N against N counted), which only the exact re-score gives, and
    every row equals the bit-profile kernel's own."""
    from deepreadmapper_amd import WindowTable, rerank_arrays
    refs, batches, want = flag_cases
    nb, q, ql = batches[placement]
    t = WindowTable(refs)
    got = _chunked_and_whole(t, lambda: rerank_arrays(t, nb, (q, ql), 1, FLAG_NC, FLAG_NC))
    t.free()
    oracle_rows, bit_rows = want[placement]
    _check(got, oracle_rows, FLAG_NC)
    for x, y in zip(got, bit_rows):
        assert np.array_equal(x, y)
    where = PLACEMENTS[placement]
    assert (got[0][where, 0] == WIN).all()
    others = np.setdiff1d(np.arange(FLAG_NQ), where)
    assert (got[1][others] < 48).all()  # no other list reaches a window with N: nothing else was flagged


# ------------------------------------------------------------------------------------------ 3. other layouts
def test_64_byte_queries_across_a_chunk_edge():
    """sw_score_f16_kernel<64> and <64, true>: tagged 64-byte queries, 130 of them in chunks of 48 (48 + 48 + 34), one
    flagged query on each side of the first edge"""
    from deepreadmapper_amd import WindowTable, rerank_arrays
    rng = np.random.default_rng(82_000)
    refs = G.windows(rng, WIN, n_dna=64, n_alpha=0)
    refs[48:, 100] = ord("N")
    (q, ql), own = _tagged_reads(rng, refs, 130, cols=62)
    assert q.shape[1] == 64
    nb = rng.integers(0, 48, size=(130, 72)).astype(np.int64)
    nb[:, 0] = own
    for i, w in ((47, 50), (48, 51)):
        q[i, 1:63] = refs[w, 70:132]
        nb[i, 0] = w
    rc, sc, ids, cnt = O.post_process_sw_static(nb, refs, WIN, q, ql, 1, 5, 72)
    assert rc == 0
    t = WindowTable(refs)
    got = _chunked_and_whole(t, lambda: rerank_arrays(t, nb, (q, ql), 1, 5, 72), chunk=48)
    t.free()
    _check(got, (sc, ids, cnt), 5)
    assert (got[0][[47, 48], 0] == 62).all()


@pytest.mark.parametrize("stride", [1, 2])
def test_dynamic_lookup_across_a_chunk_edge(stride):
    """the genome handle (windows cut from the genome, reverse-complemented for odd ids), dense and stride 2: 100
    queries in chunks of 48; the genome holds a few N, so some queries are flagged"""
    from deepreadmapper_amd import GenomeTable, rerank_dynamic_arrays
    from deepreadmapper_amd.rerank import pack_queries
    rng = np.random.default_rng(83_000 + stride)
    g = G.dna(rng, 3001)
    g[rng.integers(0, len(g), size=12)] = ord("N")
    nq, kk = 100, 40
    reads = []
    for i in range(nq):
        o = int(rng.integers(0, len(g) - 150 + 1))
        reads.append(b"<" + bytes(g[o:o + 150]) + b">")
    q, ql = pack_queries(reads)
    hi = 2 * (len(g) - WIN + 1) if stride == 1 else len(g) // 2 - 1
    nb = rng.integers(1, hi, size=(nq, kk)).astype(np.int64)
    k = 5 if stride == 1 else 60
    rc, sc, ids, cnt = O.post_process_sw_dynamic(nb, g, WIN, q, ql, stride, k, kk)
    assert rc == 0
    t = GenomeTable(g, WIN)
    got = _chunked_and_whole(t, lambda: rerank_dynamic_arrays(t, nb, (q, ql), stride, k, kk), chunk=48)
    t.free()
    _check(got, (sc, ids, cnt), k)


@pytest.mark.parametrize("stride", [2, 3, 4])
def test_sparse_stride_across_a_chunk_edge(stride):
    """the static table's sparse expansion (2 stride - 1 windows per label): 100 queries in chunks of 48"""
    from deepreadmapper_amd import WindowTable, rerank_arrays
    rng = np.random.default_rng(84_000 + stride)
    n_ref, nq, kk = 200, 100, 20
    refs = G.windows(rng, WIN, n_dna=n_ref, n_alpha=0)
    nb = rng.integers(0, n_ref // stride + 2, size=(nq, kk)).astype(np.int64)  # a few labels past the table: dropped
    nb[:, 0] = rng.integers(1, (n_ref - stride) // stride, size=nq)
    (q, ql), _ = _tagged_reads(rng, refs, nq)
    for i in range(nq):
        q[i, 1:151] = refs[nb[i, 0] * stride]
    k = kk  # every label in range gives at least one window
    rc, sc, ids, cnt = O.post_process_sw_static(nb, refs, WIN, q, ql, stride, k, kk)
    assert rc == 0
    t = WindowTable(refs)
    got = _chunked_and_whole(t, lambda: rerank_arrays(t, nb, (q, ql), stride, k, kk), chunk=48)
    t.free()
    _check(got, (sc, ids, cnt), k)
    assert (got[0][:, 0] == WIN).all()


def test_the_librarys_own_plan():
    """`sw_chunk = -1` (a new handle's value): calls of 131,072 queries and more are chunked by the library's plan.
    140,000 queries of 8 bases, two candidates each, windows of 8: a half chunk of 9,664, six of 19,328 and a last one
    of 14,368. The queries on both sides of the first two edges, the first of the last chunk and the call's last one hold
    an N, as does one of their windows, so each of those chunks has a list of its own to re-score."""
    from deepreadmapper_amd import WindowTable, rerank_arrays
    rng = np.random.default_rng(86_000)
    nq = 140_000
    refs = G.dna(rng, 64, 8)
    refs[60:, 3] = ord("N")
    q = refs[rng.integers(0, 60, size=nq)].copy()
    q[::3, 5] = ord("A")  # a third of them one base off
    nb = rng.integers(0, 60, size=(nq, 2)).astype(np.int64)
    flagged = [9_663, 9_664, 28_991, 28_992, 125_632, nq - 1]
    for j, i in enumerate(flagged):
        q[i] = refs[60 + j % 4]
        nb[i, j % 2] = 60 + j % 4
    ql = np.full(nq, 8, np.int32)
    rc, sc, ids, cnt = O.post_process_sw_static(nb, refs, 8, q, ql, 1, 2, 2)
    assert rc == 0
    t = WindowTable(refs)
    got = _chunked_and_whole(t, lambda: rerank_arrays(t, nb, (q, ql), 1, 2, 2), chunk=-1)
    t.free()
    _check(got, (sc, ids, cnt), 2)
    assert (got[0][flagged, 0] == 8).all()  # N against N counted: the exact re-score ran


# ------------------------------------------------------------------------------------------ 4. the caller's stream
@pytest.mark.parametrize("chunks", [(CHUNK, CHUNK), (CHUNK, 0), (0, CHUNK)])
def test_two_calls_on_one_stream(chunks):
    """Two calls back to back on one stream, different lists, separate outputs, one synchronise at the end: both
    equal the oracle. The calls share the handle's workspace (candidate scores, ids, counts and the flagged lists), so
    the second call's scoring must stay behind the first call's last top-k whichever way either call is launched."""
    from deepreadmapper_amd import WindowTable
    from deepreadmapper_amd._native import check, lib
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    refs, nb1, q, ql, want1 = _edge_case(128)
    nq, k = len(nb1), 128
    rng = np.random.default_rng(85_000)
    nb2 = np.ascontiguousarray(nb1[:, ::-1])  # the same windows in reverse order: other ties, other ids per rank
    nb2[:, 5] = rng.integers(0, len(refs), size=nq)
    rc, sc2, ids2, cnt2 = O.post_process_sw_static(nb2, refs, WIN, q, ql, 1, k, k)
    assert rc == 0
    t = WindowTable(refs)
    st = Stream()
    d_q, d_ql = DeviceBuffer.from_host(q), DeviceBuffer.from_host(ql)
    outs = []
    for nb, chunk in zip((nb1, nb2), chunks):
        d_nb = DeviceBuffer.from_host(nb)
        o = (DeviceBuffer((nq, k), np.int32), DeviceBuffer((nq, k), np.uint64), DeviceBuffer(nq, np.int32))
        t.sw_chunk = chunk
        check(lib().drm_post_process_sw_static_device(t.handle, d_nb.ptr, nq, k, d_q.ptr, d_ql.ptr, q.shape[1], 1, k, k,
                                                      o[0].ptr, o[1].ptr, o[2].ptr, st.handle))
        outs.append((d_nb, o))
    st.synchronize()
    for (_, o), want in zip(outs, (want1, (sc2, ids2, cnt2))):
        _check(tuple(b.download() for b in o), want, k)
    t.free()


# ------------------------------------------------------------------------------------------ 5. handle lifetime
def test_handles_made_and_freed_in_a_row():
    """six handles one after the other, each running a chunked call (which makes its streams and events) and freed;
    the last one's rows are still the oracle's"""
    from deepreadmapper_amd import WindowTable, rerank_arrays
    refs, nb, q, ql, want = _edge_case(64)
    for i in range(6):
        t = WindowTable(refs)
        t.sw_chunk = CHUNK
        got = rerank_arrays(t, nb, (q, ql), 1, 64, 64)
        t.free()
    _check(got, want, 64)
