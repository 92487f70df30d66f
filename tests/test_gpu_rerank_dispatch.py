"""Every kernel `launch_sw_rerank` (sw_rerank.hip) can pick, each compared bit for bit with the oracle (counts, scores
and ids in order, as test_gpu_parity._rerank_both does). The launcher chooses by the batch's longest query
(`pick_lq`: <= 64, <= 152, <= 256 bytes, longer refused), by the window length and the candidate count (the top-k
element is 16 bits wide when the windows are at most 255 long and a query has at most 256 candidates), and hands the
queries the class-profile kernel flags to the bit-profile kernel:
* query lengths on both sides of 64, 152 and 256 bytes, alone and mixed, against windows of 150 and 300 bytes;
* window lengths on both sides of 160 and 256 (the 16-byte block prefetch, the one-row remainder of an odd length),
  with N runs in the windows' last block that flag the queries holding N;
* scores of 255 and 256 and candidate indices 255 and 256 through the top-k kernel;
* dense lists of 129 to 1024 candidates, repeats and dropped ids among them, 1025 refused;
* the sparse fan-out up to 1023 candidates, refused just past 1024, and brought back under it by clipping;
* the dynamic lookup over the same query and window lengths;
* 65,600 queries: flagged queries past index 65,536, which only the bit-profile kernel's grid stride reaches;
* the bit-profile kernel on whole batches (DRM_SW_BITPROFILE=1, read once per process: a child process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rerank_cases as G
from oracle import oracle as O

pytestmark = pytest.mark.gpu

NQ = 24  # queries per case, against 64 windows (48 DNA, 16 over a 40-letter alphabet)
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sw_bitprofile_child.py")


def _static_both(refs, nb, reads, stride, k, kc, table=None):
    """the rerank on the GPU against the oracle; returns the GPU's (scores, ids, counts)"""
    from deepreadmapper_amd import WindowTable, rerank_arrays
    from deepreadmapper_amd.rerank import pack_queries
    qbuf, ql = reads if isinstance(reads, tuple) else pack_queries(reads)
    rc, sc_o, id_o, cnt_o = O.post_process_sw_static(nb, refs, refs.shape[1], qbuf, ql, stride, k, kc)
    assert rc == 0
    t = table if table is not None else WindowTable(refs)
    sc, ids, cnt = rerank_arrays(t, nb, (qbuf, ql), stride, k, kc)
    if table is None:
        t.free()
    assert np.array_equal(cnt, cnt_o)
    m = np.arange(k)[None] < cnt[:, None]
    bad = np.flatnonzero(((sc != sc_o) & m).any(axis=1) | ((ids != id_o) & m).any(axis=1))
    assert bad.size == 0, f"{bad.size} queries differ from the oracle, first {bad[:8]}"
    return sc, ids, cnt


def _refused(fn):
    from deepreadmapper_amd._native import DRM_ERR_UNSUPPORTED, DrmError
    with pytest.raises(DrmError) as e:
        fn()
    assert e.value.code == DRM_ERR_UNSUPPORTED, str(e.value)


# ------------------------------------------------------------------------------------------ 1. query length
@pytest.mark.parametrize("win_len", [150, 300])
@pytest.mark.parametrize("qlen", [64, 65, 152, 153, 154, 200, 255, 256])
def test_query_length(qlen, win_len):
    """One-length batches and batches whose longest query is `qlen` bytes: 64 | 65 and 152 | 153 are the two sides of
    pick_lq's switches, 153 to 256 take sw_score_kernel<256> (full mode) for every query of the batch."""
    rng = np.random.default_rng(10_000 + 10 * qlen + win_len)
    refs = G.windows(rng, win_len)
    reads, own = G.byte_reads(rng, refs, [qlen] * NQ)
    _static_both(refs, G.lists(rng, own, len(refs), 72), reads, 1, 72, 72)  # 72: lanes 0-7 hold two candidates
    lengths = rng.integers(3, qlen + 1, size=NQ)
    lengths[int(rng.integers(0, NQ))] = qlen
    reads, own = G.byte_reads(rng, refs, lengths)
    _static_both(refs, G.lists(rng, own, len(refs), 72), reads, 1, 5, 72)


@pytest.mark.parametrize("win_len", [150, 300])
def test_query_lengths_mixed_to_256(win_len):
    """queries of 20, 150 and 256 bytes in one batch: all of them go to <256>"""
    rng = np.random.default_rng(11_000 + win_len)
    refs = G.windows(rng, win_len)
    reads, own = G.byte_reads(rng, refs, [20, 150, 256] * (NQ // 3))
    _static_both(refs, G.lists(rng, own, len(refs), 72), reads, 1, 72, 72)


def test_query_of_257_bytes_is_refused():
    """pick_lq refuses a batch with a 257-byte query (DRM_ERR_UNSUPPORTED); the next call on the table succeeds"""
    from deepreadmapper_amd import WindowTable, rerank_arrays
    rng = np.random.default_rng(12_000)
    refs = G.windows(rng, 150)
    t = WindowTable(refs)
    reads, own = G.byte_reads(rng, refs, [150] * 7 + [257] + [256] * 4)
    nb = G.lists(rng, own, len(refs), 24)
    _refused(lambda: rerank_arrays(t, nb, reads, 1, 5, 24))
    reads[7] = reads[7][:256]
    _static_both(refs, nb, reads, 1, 5, 24, table=t)
    t.free()


# ------------------------------------------------------------------------------------------ 2. window length
@pytest.mark.parametrize("win_len", [151, 159, 160, 161, 255, 256, 257, 300])
def test_window_length(win_len):
    """Windows longer than 150: 10 to 19 blocks of 16 bytes, the last one partial or (160, 256) full, odd lengths
    ending in the one-row remainder; against reads of 42, 152 and 256 bytes. Of each such batch the tagged DNA reads
    (a third) have 40 and 150 DP columns, the <64> and <150> class-profile kernels; the untagged ones have 42 and 152
    columns (152 are flagged for the bit-profile kernel) and a third are over the 40-letter alphabet. Then windows
    with a run of N in their last block and reads cut from the windows' ends: a read that holds N is flagged and scored
    again by the bit-profile kernel (<64, true>, <152, true>); these reads are all tagged, 40 and 150 columns."""
    rng = np.random.default_rng(20_000 + win_len)
    refs = G.windows(rng, win_len)
    for qlen in (42, 152, 256):
        reads, own = G.byte_reads(rng, refs, [qlen] * NQ)
        _static_both(refs, G.lists(rng, own, len(refs), 72), reads, 1, 72, 72)
    last = 16 * ((win_len - 1) // 16)  # start of the last 16-byte block
    refs = G.windows(rng, win_len, n_alpha=0)
    for i in range(0, len(refs), 2):
        lo = int(rng.integers(last, win_len))
        refs[i, lo:int(rng.integers(lo, win_len)) + 1] = ord("N")
    for cols in (40, 150):
        reads = [b"<" + bytes(refs[i % len(refs), win_len - cols:]) + b">" for i in range(NQ)]
        assert sum(b"N" in r for r in reads) >= NQ // 3
        nb = G.lists(rng, np.arange(NQ) % len(refs), len(refs), 72)
        sc, _, _ = _static_both(refs, nb, reads, 1, 72, 72)
        assert (sc[:, 0] == cols).all()  # the read's own window, N against N counted


# ------------------------------------------------------------------------------------------ 3. top-k element width
@pytest.mark.parametrize("k", ["all", 5])
@pytest.mark.parametrize("win_len,ncand", [(255, 256), (255, 257), (256, 256), (256, 257)])
def test_topk_element_width(win_len, ncand, k):
    """sw_topk_kernel packs (score << 8) | index into 16 bits when the windows are at most 255 long and the lists at
    most 256: reads of 256 bases that contain their window score the window length (255 | 256), and the read's own
    window is the LAST candidate of its list (index 255 | 256) and nowhere else in it, so both fields meet their edge
    in the element that must come out on top."""
    rng = np.random.default_rng(30_000 + 10 * win_len + ncand)
    refs = G.windows(rng, win_len, n_alpha=0)
    nq = 16
    reads = []
    for i in range(nq):
        r = G.dna(rng, 256)
        o = int(rng.integers(0, 256 - win_len + 1))
        r[o:o + win_len] = refs[i]
        reads.append(bytes(r))
    nb = rng.integers(nq, len(refs), size=(nq, ncand)).astype(np.int64)  # windows 16.. : none of the reads' own
    nb[:, -1] = np.arange(nq)
    k = ncand if k == "all" else k
    sc, ids, cnt = _static_both(refs, nb, reads, 1, k, ncand)
    assert (cnt == k).all()
    assert (sc[:, 0] == win_len).all() and (sc[:, 1:] < win_len).all()  # a score of 255 | 256 is reached, once
    assert (ids[:, 0] == np.arange(nq)).all()  # by the candidate at index ncand - 1


# ------------------------------------------------------------------------------------------ 4. candidate counts
@pytest.mark.parametrize("ncand", [129, 191, 192, 193, 256, 257, 512, 1024])
def test_dense_candidate_counts(ncand):
    """Dense lists of more than 128 candidates for reads of 42 bytes (<64>; the tagged third of the batch has 40
    columns), 152 bytes (<150> for the tagged reads' 150 columns, the bit-profile kernel for the untagged 152) and 200
    bytes (<256>):
    2 to 8 passes of 128 candidates per wave, the last one with no, some or all second halves; 7 ids that are out of
    range are dropped (at 1024 the 1031 ids take the one-thread list builder, not the ballot compaction)."""
    rng = np.random.default_rng(40_000 + ncand)
    refs = G.windows(rng, 150)
    nq = 8 if ncand >= 512 else 12
    for qlen in (42, 152, 200):
        reads, own = G.byte_reads(rng, refs, [qlen] * nq)
        nb = G.dense_lists(rng, own, len(refs), ncand, 7)
        sc, ids, cnt = _static_both(refs, nb, reads, 1, ncand, ncand + 7)
        assert (cnt == ncand).all() and (ids < len(refs)).all()
        _static_both(refs, nb, reads, 1, 5, ncand + 7)
    reads, own = G.byte_reads(rng, refs, [152] * nq)
    _static_both(refs, G.dense_lists(rng, own, len(refs), ncand, 0), reads, 1, 5, ncand)  # every id in range


def test_dense_1025_candidates_are_refused():
    """1025 in-range candidates are past the kernels' cap of 1024: DRM_ERR_UNSUPPORTED for the call (the reference
    has no cap, so this is a loud failure, not parity), also when only some queries of the batch are over it; the
    handle stays usable."""
    from deepreadmapper_amd import WindowTable, rerank_arrays
    rng = np.random.default_rng(41_000)
    refs = G.windows(rng, 150)
    t = WindowTable(refs)
    for qlen in (42, 152, 200):
        reads, own = G.byte_reads(rng, refs, [qlen] * 6)
        nb = G.dense_lists(rng, own, len(refs), 1025, 0)
        _refused(lambda: rerank_arrays(t, nb, reads, 1, 5, 1025))
        nb[3, 77] = -1  # one query back at 1024: the others still refuse the call
        _refused(lambda: rerank_arrays(t, nb, reads, 1, 5, 1025))
        _static_both(refs, nb[:, :1024], reads, 1, 5, 1024, table=t)
    t.free()


# ------------------------------------------------------------------------------------------ 5. sparse fan-out
def _sparse_case(seed, n_ref, stride, kk, nq=8, lo=1, hi=None):
    rng = np.random.default_rng(seed)
    refs = G.windows(rng, 150, n_dna=n_ref, n_alpha=0)
    hi = (n_ref - stride) // stride if hi is None else hi  # id * stride + stride <= n_ref: nothing clipped
    nb = rng.integers(lo, hi + 1, size=(nq, kk)).astype(np.int64)
    own = nb[:, 0] * stride
    reads = [G.dna_read(rng, refs, int(own[i]), 150, True, n_dna=n_ref)[0] for i in range(nq)]
    return refs, nb, reads


@pytest.mark.parametrize("stride,kk", [(2, 341), (4, 146), (8, 68)])
def test_sparse_fanout_to_the_cap(stride, kk):
    """kk labels x (2 stride - 1) windows each = 1023 | 1022 | 1020 candidates, ids away from both table ends"""
    refs, nb, reads = _sparse_case(50_000 + stride, 200, stride, kk)
    n = kk * (2 * stride - 1)
    sc, ids, cnt = _static_both(refs, nb, reads, stride, n, kk)
    assert (cnt == n).all()
    _static_both(refs, nb, reads, stride, 5, kk)


@pytest.mark.parametrize("stride,kk", [(2, 342), (4, 147), (8, 69)])
def test_sparse_fanout_past_the_cap(stride, kk):
    """1026 | 1029 | 1035 candidates: refused (status -2 -> DRM_ERR_UNSUPPORTED), the handle stays usable; with ids at
    both table ends the clipped expansion of the same number of labels is back under 1024 and equals the oracle"""
    from deepreadmapper_amd import WindowTable, rerank_arrays
    n_ref = 197  # 197 = 8 * 24 + 5: the last label's expansion is clipped at every stride
    refs, nb, reads = _sparse_case(51_000 + stride, n_ref, stride, kk)
    assert kk * (2 * stride - 1) > 1024
    t = WindowTable(refs)
    _refused(lambda: rerank_arrays(t, nb, reads, stride, 5, kk))
    one = nb.copy()
    one[1:, :8] = 0  # every query but the first is clipped back under the cap: the call is still refused
    _refused(lambda: rerank_arrays(t, one, reads, stride, 5, kk))
    clipped = nb.copy()
    top = (n_ref - 1) // stride  # the last label whose centre lies in the table
    clipped[:, 1:9:2] = 0  # expands to [0, stride): stride - 1 windows lost each
    clipped[:, 2:10:2] = top  # [top * stride - stride + 1, 197): clipped at the table's end
    n = _expanded(clipped[0], stride, n_ref)
    assert n <= 1024 and all(_expanded(r, stride, n_ref) == n for r in clipped)
    sc, ids, cnt = _static_both(refs, clipped, reads, stride, n, kk, table=t)
    assert (cnt == n).all()
    _static_both(refs, clipped, reads, stride, 5, kk, table=t)
    t.free()


def _expanded(labels, stride, n_ref):
    """candidates of one sparse list: find_sequences' clipped expansion (post_processor.cpp:238-335)"""
    n = 0
    for i in map(int, labels):
        a = i * stride
        if 0 <= a < n_ref:
            n += min(a + stride, n_ref) - max(a - stride + 1, 0)
    return n


# ------------------------------------------------------------------------------------------ 6. dynamic lookup
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGTN")] = list(b"TGCAN")


def _dyn_both(g, ref_len, nb, reads, stride, k, kc):
    from deepreadmapper_amd import GenomeTable, rerank_dynamic_arrays
    from deepreadmapper_amd.rerank import pack_queries
    q, ql = pack_queries(reads)
    rc, sco, ido, cnto = O.post_process_sw_dynamic(nb, g, ref_len, q, ql, stride, k, kc)
    assert rc == 0
    t = GenomeTable(g, ref_len)
    sc, ids, cnt = rerank_dynamic_arrays(t, nb, (q, ql), stride, k, kc)
    t.free()
    assert np.array_equal(cnt, cnto)
    m = np.arange(k)[None] < cnt[:, None]
    assert np.array_equal(sc[m], sco[m]) and np.array_equal(ids[m], ido[m])
    return sc, ids


def _genome_reads(rng, g, lengths):
    """reads cut from the genome, odd ones reverse-complemented, every third one tagged; length in bytes"""
    out = []
    for i, n in enumerate(lengths):
        tags = i % 3 == 0
        cols = int(n) - 2 * tags
        o = int(rng.integers(0, len(g) - cols + 1))
        r = g[o:o + cols]
        r = bytes(COMP[r[::-1]] if i % 2 else r)
        out.append(b"<" + r + b">" if tags else r)
    return out


@pytest.mark.parametrize("ref_len,qlen", [(150, 153), (150, 200), (150, 256), (151, 152), (256, 152), (300, 152),
                                          (151, 42), (256, 42), (300, 42), (300, 256)])
def test_dynamic_lookup(ref_len, qlen):
    """The dynamic lookup (windows cut from a 3,001-base genome with a few N, one byte per DP row, reverse-complemented
    for odd ids) over the query lengths that take <256> and the window lengths past 150: dense lists with the ids -1,
    past the genome end and the last reverse-complement window, and the stride-2 expansion."""
    rng = np.random.default_rng(60_000 + 10 * ref_len + qlen)
    g = G.dna(rng, 3001)
    g[rng.integers(0, len(g), size=12)] = ord("N")
    nwin = 2 * (len(g) - ref_len + 1)
    reads = _genome_reads(rng, g, [qlen] * NQ)
    nb = rng.integers(0, nwin, size=(NQ, 72)).astype(np.int64)
    nb[:, 0] = nwin - 1  # the last reverse-complement window
    nb[:, 1] = 0
    nb[::3, 5] = -1  # faiss padding: kept, an empty window, id 2^64 - 1
    nb[::4, 9] = nwin + 17  # past the genome end: kept, an empty window
    sc, ids = _dyn_both(g, ref_len, nb, reads, 1, 72, 72)
    assert (ids == np.uint64(2 ** 64 - 1)).any() and (sc[ids == np.uint64(2 ** 64 - 1)] == 0).all()
    _dyn_both(g, ref_len, nb, reads, 1, 5, 40)
    nb = rng.integers(1, len(g) // 2 - 1, size=(NQ, 24)).astype(np.int64)  # stride 2: label * 2 is a window id
    nb[::5, 3] = -1  # dropped
    nb[::6, 4] = len(g) // 2 + 3  # past the genome length: dropped
    nb[::7, 6] = len(g) // 2  # 3000 < 3001: the expansion [2999, 3002) is clipped to the genome length
    _dyn_both(g, ref_len, nb, reads, 2, 5, 24)
    _dyn_both(g, ref_len, nb, reads, 2, 60, 24)


# ------------------------------------------------------------------------------------------ 7. past 65,536 queries
@pytest.mark.parametrize("long_query", [0, 100])
def test_flagged_queries_past_65536(long_query):
    """sw_score_kernel runs min(nq, 65536) workgroups and strides over the rest: of 65,600 queries of 8 bases (two
    candidates each, windows of 8) the queries 3, 65,540 and 65,599 hold an N and so does one of their windows, so the
    class-profile kernel flags them and only the stride of the ONLY_FLAGGED pass reaches the last two. pick_lq takes
    the batch maximum: all queries of 8 bytes run sw_score_f16_kernel<64> and <64, true>; with one unflagged query of
    100 bytes in the (widened) buffer the same batch runs sw_score_f16_kernel<150> and <152, true>."""
    rng = np.random.default_rng(70_000)
    nq = 65_600
    refs = G.dna(rng, 64, 8)
    refs[60:, 3] = ord("N")
    q = np.zeros((nq, max(8, long_query)), np.uint8)
    q[:, :8] = refs[rng.integers(0, 60, size=nq)]
    q[::3, 5] = ord("A")  # a third of them one base off
    nb = rng.integers(0, 60, size=(nq, 2)).astype(np.int64)
    flagged = [3, 65_540, 65_599]
    for j, i in enumerate(flagged):
        q[i, :8] = refs[60 + j]  # N at column 3, against ...
        nb[i, j % 2] = 60 + j  # ... its own window, first or second in the list
    ql = np.full(nq, 8, np.int32)
    if long_query:
        q[7] = G.dna(rng, long_query)
        q[7, 40:48] = refs[nb[7, 0]]
        ql[7] = long_query
    sc, ids, cnt = _static_both(refs, nb, (q, ql), 1, 2, 2)
    assert (cnt == 2).all() and (sc[flagged, 0] == 8).all()  # N against N counted: the exact re-score ran
    assert not long_query or sc[7, 0] == 8


# ------------------------------------------------------------------------------------------ 8. bit-profile kernel
def test_bitprofile_kernel_on_whole_batches(tmp_path):
    """DRM_SW_BITPROFILE=1 sends every query of a batch to sw_score_kernel<64> / <152> (full mode). The launcher reads
    the variable once per process, so the fixed cases of rerank_cases.cases() run in one fresh child
    (sw_bitprofile_child.py); its rows equal the oracle's and the default kernels', computed here. A child that hangs
    is killed at its time limit and fails the test; whoever runs the suite should then stop there and not start further
    GPU work behind a hung process."""
    assert os.environ.get("DRM_SW_BITPROFILE", "0") in ("", "0")  # this process runs the default kernels
    out = str(tmp_path / "bitprofile.npz")
    argv = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, out]
    r = subprocess.run(argv, env=dict(os.environ, DRM_SW_BITPROFILE="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(out)
    for name, refs, nb, reads, stride, k, kc in G.cases():
        sc, ids, cnt = _static_both(refs, nb, reads, stride, k, kc)  # default kernels == oracle
        m = np.arange(k)[None] < cnt[:, None]
        assert np.array_equal(got[name + ".counts"], cnt), name
        assert np.array_equal(got[name + ".scores"][m], sc[m]) and np.array_equal(got[name + ".ids"][m], ids[m]), name
