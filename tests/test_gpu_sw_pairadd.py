"""The SW rerank's scoring kernel forms the diagonal terms of two adjacent columns with one 64-bit add
(sw_rows_i16 in sw_rerank.hip: the pair is read at an odd column, its high word is carried one step). The shapes
here are the smallest at which that pairing can go wrong, each compared bit for bit with the oracle as
test_gpu_parity._rerank_both does:
* query columns 1-5 (column 0 has no add, column 1 the lone 32-bit add, 2-3 the first pair, a trailing column
  without a partner), 63-65 (the two sides of the <64> instantiation) and 149-150, with and without the "<" ">" tags;
* window lengths 1-3 and 149-150 (odd lengths end in the one-row remainder);
* 1, 2, 63-65 and 128 candidates per query (the second candidate of a lane absent, mixed, present);
* carries: the four 16-bit halves of one 64-bit add hold two candidates x two columns, so a window equal to the read
  sits beside an unrelated one in the other half of the register, at every lane, either way round, and an all-A
  read meets all-A windows (every cell a match, 150 reached in every column of both halves);
* the dynamic lookup (windows cut from a genome, forward and reverse-complement ids) over the same lengths."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
NQ = 24  # queries per case (at most 48), against 48 windows at most


def _dna(rng, *shape):
    return rng.choice(ACGT, size=shape).astype(np.uint8)


def _windows(rng, n=48, length=150):
    return _dna(rng, n, length)


def _reads_from(rng, refs, n, cols, tags):
    """n reads of `cols` bases cut from the windows (every third one with a few substitutions, every fifth one
    unrelated), so that the best alignment runs through every column; tagged like format_fastq when asked."""
    out = []
    for i in range(n):
        w = refs[i % len(refs)]
        if i % 5 == 4:
            r = _dna(rng, cols)
        elif refs.shape[1] < cols:  # a short window: the read holds it whole
            o = int(rng.integers(0, cols - refs.shape[1] + 1))
            r = _dna(rng, cols)
            r[o:o + refs.shape[1]] = w
        else:
            o = int(rng.integers(0, refs.shape[1] - cols + 1))
            r = w[o:o + cols].copy()
            if i % 3 == 2:
                for p in rng.integers(0, cols, size=max(1, cols // 20)):
                    r[p] = ACGT[(int(np.searchsorted(ACGT, r[p])) + 1) % 4]
        out.append((b"<" + bytes(r) + b">") if tags else bytes(r))
    return out


def _rerank_both(refs, nb, reads, k, kc):
    from deepreadmapper_amd import WindowTable, rerank_arrays
    from deepreadmapper_amd.rerank import pack_queries
    qbuf, ql = pack_queries(reads)
    rc, sc_o, id_o, cnt_o = O.post_process_sw_static(nb, refs, refs.shape[1], qbuf, ql, 1, k, kc)
    assert rc == 0
    t = WindowTable(refs)
    sc, ids, cnt = rerank_arrays(t, nb, (qbuf, ql), 1, k, kc)
    t.free()
    assert np.array_equal(cnt, cnt_o)
    for i in range(len(nb)):
        n = cnt[i]
        assert np.array_equal(sc[i, :n], sc_o[i, :n]) and np.array_equal(ids[i, :n], id_o[i, :n]), i
    return sc


def _lists(rng, nq, n_ref, ncand):
    """Candidate lists: the read's own window first, then random ones (repeats allowed, as the search may give)."""
    nb = rng.integers(0, n_ref, size=(nq, ncand)).astype(np.int64)
    nb[:, 0] = np.arange(nq) % n_ref
    return nb


@pytest.mark.parametrize("tags", [False, True])
@pytest.mark.parametrize("cols", [1, 2, 3, 4, 5, 63, 64, 65, 149, 150])
def test_query_columns(cols, tags):
    rng = np.random.default_rng(1000 + cols)
    refs = _windows(rng)
    reads = _reads_from(rng, refs, NQ, cols, tags)
    _rerank_both(refs, _lists(rng, NQ, len(refs), 72), reads, 72, 72)  # 72: lanes 0-7 hold two candidates


@pytest.mark.parametrize("ref_len", [1, 2, 3, 149, 150])
def test_window_lengths(ref_len):
    rng = np.random.default_rng(2000 + ref_len)
    refs = _windows(rng, 48, ref_len)
    for cols in (150, 40):  # the <150> and the <64> instantiation
        reads = _reads_from(rng, refs, NQ, cols, True)
        _rerank_both(refs, _lists(rng, NQ, len(refs), 72), reads, 72, 72)


@pytest.mark.parametrize("ncand", [1, 2, 63, 64, 65, 128])
def test_candidates_per_query(ncand):
    rng = np.random.default_rng(3000 + ncand)
    refs = _windows(rng)
    for cols in (150, 62):
        reads = _reads_from(rng, refs, NQ, cols, True)
        _rerank_both(refs, _lists(rng, NQ, len(refs), ncand), reads, ncand, ncand)


@pytest.mark.parametrize("cols", [150, 149, 64, 63])
def test_carry_stress(cols):
    """Lane l scores candidates l (low halves) and l + 64 (high halves). Window i < 8 equals read i in its first
    `cols` bytes; the other windows are unrelated to every read; window 47 is all A and read 8 is all A."""
    rng = np.random.default_rng(4000 + cols)
    refs = _windows(rng)
    refs[47] = ord("A")
    reads = [bytes(refs[i, :cols]) for i in range(8)] + [b"A" * cols]
    nq = len(reads)
    own = np.arange(nq, dtype=np.int64)[:, None]
    own[8] = 47
    other = 8 + (np.arange(nq)[:, None] + np.arange(64)[None]) % 39  # windows 8..46
    eq = np.broadcast_to(own, (nq, 64))
    even = (np.arange(64) % 2 == 0)[None]
    for lo, hi in ((eq, other), (other, eq), (np.where(even, eq, other), np.where(even, other, eq)), (eq, eq)):
        nb = np.concatenate([lo, hi], axis=1).astype(np.int64)
        sc = _rerank_both(refs, nb, reads, 128, 128)
        assert (sc[:, :64] == cols).all()  # the read's own window, found at every lane position it was put in
    allA = np.full((1, 128), 47, np.int64)  # every cell of both halves a match
    sc = _rerank_both(refs, allA, [b"<" + b"A" * cols + b">"], 128, 128)
    assert (sc == min(cols, 150)).all()


def _dyn_both(g, ref_len, nb, reads, k, kc):
    from deepreadmapper_amd import GenomeTable, rerank_dynamic_arrays
    from deepreadmapper_amd.rerank import pack_queries
    q, ql = pack_queries(reads)
    rc, sco, ido, cnto = O.post_process_sw_dynamic(nb, g, ref_len, q, ql, 1, k, kc)
    assert rc == 0
    t = GenomeTable(g, ref_len)
    sc, ids, cnt = rerank_dynamic_arrays(t, nb, (q, ql), 1, k, kc)
    t.free()
    assert np.array_equal(cnt, cnto) and np.array_equal(sc, sco) and np.array_equal(ids, ido)


@pytest.mark.parametrize("ref_len", [1, 2, 3, 149, 150])
def test_dynamic_lookup_lengths(ref_len):
    rng = np.random.default_rng(5000 + ref_len)
    g = _dna(rng, 420)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    nwin = 2 * (len(g) - ref_len + 1)
    for cols in (150, 60):
        reads = []
        for i in range(NQ):
            o = int(rng.integers(0, len(g) - cols + 1))
            r = g[o:o + cols]
            reads.append(b"<" + bytes(comp[r[::-1]] if i % 2 else r) + b">")
        nb = rng.integers(0, nwin, size=(NQ, 72)).astype(np.int64)
        nb[:, 0] = nwin - 1  # the last reverse-complement window
        nb[:, 1] = 0
        _dyn_both(g, ref_len, nb, reads, 72, 72)
