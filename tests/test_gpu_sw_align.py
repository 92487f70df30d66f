"""GPU tests of the Smith-Waterman alignment (sw_align.hip, drm_sw_align): records and operations equal the
Python restatement of the definition (tests/sw_align_ref.py) on every pair, through both handle kinds, the
Python wrapper, drm_sam_cigar and the DRM_SAM_CIGAR mode of bin/pipeline."""
import os
import re
import subprocess

import numpy as np
import pytest

import sw_align_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ACGT = list(b"ACGT")


def _check(rec, ops, p, w, q):
    """Pair p of a wrapper result equals the restatement on (w, q)."""
    want, wops = R.align(w, q)
    got = {f: int(rec[f][p]) for f in R.FIELDS}
    assert got == want, (p, w, q, got, want)
    assert [int(x) for x in ops[p]] == wops, (p, w, q)


def _table(windows):
    from deepreadmapper_amd import WindowTable
    return WindowTable(np.frombuffer(b"".join(windows), dtype=np.uint8).reshape(len(windows), len(windows[0])))


# ------------------------------------------------------------------------------------------ known answers
KNOWN = [(b"AAAAAAAA", b"<AAAA>"), (b"ACACACACAC", b"<ACAC>"), (b"AAAACCCC", b"<AAAATCCCC>"),
         (b"AAAATCCCC", b"<AAAACCCC>"), (b"GGGG", b"<TTTT>"), (b"A", b"A")]


@pytest.mark.parametrize("case", range(len(KNOWN)))
def test_known_answers(case):
    from deepreadmapper_amd import sw_align_arrays
    w, q = KNOWN[case]
    t = _table([w])
    rec, ops = sw_align_arrays(t, [0], [0], [q])
    t.free()
    _check(rec, ops, 0, w, q)
    span = tuple(int(rec[f][0]) for f in ("ref_begin", "ref_end", "q_begin", "q_end"))
    want = [((0, 4, 1, 5), "4M", 4), ((0, 4, 1, 5), "4M", 4), ((0, 8, 1, 10), "4M1I4M", 7), ((0, 9, 1, 9), "4M1D4M", 7),
            ((0, 0, 0, 0), "", 0), ((0, 1, 0, 1), "1M", 1)][case]
    assert (span, R.cigar_string(ops[0]), int(rec["score"][0])) == want
    assert int(rec["status"][0]) == (1 if case == 4 else 0)


# ------------------------------------------------------------------------------------------ shape edges
def _derive_query(rng, w, q_len):
    """A query of exactly q_len bytes derived from window w: a stretch of w (or w inside random flanks when the
    query is longer) with a few substitutions, insertions and deletions, tagged like format_fastq when it has
    room for the tags. synth.simulate_reads only substitutes, hence this generator."""
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
    while len(s) < core:  # random flanks, alternating sides
        s.insert(0 if len(s) % 2 else len(s), int(rng.choice(ACGT)))
    s = bytes(s[:core])
    return b"<" + s + b">" if q_len >= 3 else s


# q_len <= 192 runs the 3-columns-per-lane build, anything longer the 4-column one; the second group repeats
# short lengths so that both builds see ragged queries in one call
Q_GROUPS = {"lq192": [1, 2, 63, 64, 65, 128, 129, 152, 191, 192], "lq256": [193, 255, 256, 1, 65, 152]}


@pytest.mark.parametrize("group", sorted(Q_GROUPS))
@pytest.mark.parametrize("ref_len", [1, 64, 150, 256])
def test_shape_edges(ref_len, group):
    from deepreadmapper_amd import sw_align_arrays
    rng = np.random.default_rng(1000 * ref_len + len(group))
    q_lens = Q_GROUPS[group]
    windows = [bytes(rng.choice(ACGT, size=ref_len).astype(np.uint8)) for _ in range(4 * len(q_lens))]
    queries = [_derive_query(rng, windows[4 * a + b], ql) for a, ql in enumerate(q_lens) for b in range(4)]
    assert sorted({len(q) for q in queries}) == sorted(set(q_lens))
    t = _table(windows)
    n = len(windows)
    rec, ops = sw_align_arrays(t, np.arange(n), np.arange(n), queries)
    t.free()
    for p in range(n):
        _check(rec, ops, p, windows[p], queries[p])
    if ref_len >= 64:
        assert {int(x) & 15 for o in ops for x in o} == {R.M, R.I, R.D}


def test_query_longer_than_256_is_unsupported():
    from deepreadmapper_amd import DrmError, sw_align_arrays
    from deepreadmapper_amd._native import DRM_ERR_UNSUPPORTED
    t = _table([b"ACGT" * 8])
    with pytest.raises(DrmError) as e:
        sw_align_arrays(t, [0], [0], [b"A" * 257])
    assert e.value.code == DRM_ERR_UNSUPPORTED and "257" in str(e.value)
    rec, _ = sw_align_arrays(t, [0], [0], [b"ACGT" * 64])  # 256 is the limit itself
    t.free()
    assert int(rec["score"][0]) == 32


# ------------------------------------------------------------------------------------------ pair counts
@pytest.fixture(scope="module")
def short_pairs():
    """16 windows of 24 bytes x 8 queries derived from them, with the restatement of all 128 combinations."""
    rng = np.random.default_rng(5)
    windows = [bytes(rng.choice(ACGT, size=24).astype(np.uint8)) for _ in range(16)]
    queries = [_derive_query(rng, windows[2 * i], 18 + i) for i in range(8)]
    want = {(w, q): R.align(windows[w], queries[q]) for w in range(16) for q in range(8)}
    return windows, queries, want


def _grid_waves():
    import ctypes as C
    from deepreadmapper_amd._native import lib

    class Props(C.Structure):
        _fields_ = [("cu_count", C.c_int32), ("clock_khz", C.c_int32), ("total_mem", C.c_int64),
                    ("lds_per_cu", C.c_int32), ("arch", C.c_char * 64)]
    p = Props()
    assert lib().drm_device_get_props(0, C.byref(p)) == 0
    return 16 * p.cu_count  # launch_sw_align's grid bound


@pytest.mark.parametrize("npairs", [1, 63, 64, 65, "beyond_grid"])
def test_pair_counts_and_batch_position(short_pairs, npairs):
    from deepreadmapper_amd import sw_align_arrays
    windows, queries, want = short_pairs
    if npairs == "beyond_grid":  # more pairs than launched waves: the per-wave loop runs more than once
        npairs = max(5000, _grid_waves() + 37)
    # pair p = (window, query) number 37 * p mod 128: every combination comes back at many batch positions
    combo = (37 * np.arange(npairs)) % 128
    wid, pq = combo // 8, combo % 8
    t = _table(windows)
    rec, ops = sw_align_arrays(t, wid, pq, queries)
    t.free()
    assert len(rec) == npairs
    for p in range(npairs):
        r, o = want[(int(wid[p]), int(pq[p]))]
        assert {f: int(rec[f][p]) for f in R.FIELDS} == r, p
        assert [int(x) for x in ops[p]] == o, p


# ------------------------------------------------------------------------------------------ static / dynamic
def test_static_and_dynamic_handles_agree():
    from deepreadmapper_amd import GenomeTable, WindowTable, extract_fasta_sequence, sw_align_arrays, synth
    g = np.frombuffer(extract_fasta_sequence(os.path.join(GOLDEN, "ecoli_150.fna")), dtype=np.uint8).copy()
    g[400:406] = ord("N")  # the golden genome has no N: a short run, raw byte equality (N matches N)
    refs = synth.windows_lookup(g, 150, 1)
    nwin = len(refs)
    rng = np.random.default_rng(3)
    ids = [0, 1, 2 * 300, 2 * 300 + 1, 2 * 380, 2 * 390 + 1, nwin - 2, nwin - 1, nwin, nwin + 5, 2 ** 40 + 1]
    queries = []
    for w in ids:
        wb = R.window_bytes(g, 150, w)
        queries.append(_derive_query(rng, wb, 152) if wb else b"<" + bytes(rng.choice(ACGT, size=150).astype(np.uint8)) + b">")
    st, dy = WindowTable(refs), GenomeTable(g, 150)
    pq = np.arange(len(ids))
    rs, os_ = sw_align_arrays(st, ids, pq, queries)
    rd, od = sw_align_arrays(dy, ids, pq, queries)
    st.free()
    dy.free()
    assert rs.tobytes() == rd.tobytes()
    assert [list(map(int, a)) for a in os_] == [list(map(int, a)) for a in od]
    for p, w in enumerate(ids):
        wb = R.window_bytes(g, 150, w)
        if w < nwin:
            assert wb == bytes(refs[w])  # the table row and the genome slice are the same bytes
        _check(rd, od, p, wb, queries[p])
    assert [int(s) for s in rd["status"][-3:]] == [1, 1, 1]  # past the genome end / outside the table
    n_q = [q.count(b"N") for q in queries]
    assert n_q[4] > 0 and n_q[5] > 0 and int(rd["status"][4]) == 0  # the N windows were aligned through the N run


# ------------------------------------------------------------------------------------------ rerank consistency
def test_consistent_with_the_rerank(c1):
    from deepreadmapper_amd import WindowTable, calc_sw_scores, read_index, rerank_arrays, sw_align_arrays
    ix = read_index(c1["index"], 0)
    _, I, _ = ix.search(c1["q"], 128, 128)
    ix.free()
    t = WindowTable(c1["refs"])
    reads = c1["reads"]
    scores, ids, counts = rerank_arrays(t, I, reads, 1, 5, 128)
    assert (counts == 5).all()
    wid = ids.reshape(-1)
    pq = np.repeat(np.arange(len(reads)), 5)
    assert len(wid) == 750
    rec, ops = sw_align_arrays(t, wid, pq, reads)
    t.free()
    windows = [bytes(c1["refs"][int(w)]) for w in wid]
    assert np.array_equal(rec["score"], scores.reshape(-1))
    assert np.array_equal(rec["score"], calc_sw_scores(windows, [reads[int(q)] for q in pq]))
    for p in range(750):
        assert int(rec["status"][p]) == 0
        score, nm, first, last = R.replay(windows[p], reads[int(pq[p])], rec[p], ops[p])
        assert (score, nm, first, last) == (int(rec["score"][p]), int(rec["nm"][p]), True, True), p
    for p in range(0, 750, 5):  # the 150 top-1 pairs
        _check(rec, ops, p, windows[p], reads[int(pq[p])])


# ------------------------------------------------------------------------------------------ truncation
def test_truncated_operations_and_retry():
    from deepreadmapper_amd import sw_align_arrays
    from deepreadmapper_amd import rerank as RR
    w, q = b"ACGTACGTTTGACCAGTACCGTAGGCATTCAG", b"<ACGTACGTTTGACAGTACCGTAGAGCATTCAG>"  # one deletion, one insertion
    want, wops = R.align(w, q)
    assert len(wops) >= 3
    t = _table([w, w])
    qbuf, qlen = RR.pack_queries([q])
    rec, ops = RR._sw_align_call(t, np.array([0, 1], np.uint64), np.array([0, 0], np.int64), qbuf, qlen, 1)
    for p in range(2):
        assert int(rec["status"][p]) == 2 and int(rec["n_ops"][p]) == len(wops)
        assert int(ops[p, 0]) == wops[0]
        assert {f: int(rec[f][p]) for f in R.FIELDS if f != "status"} == {f: v for f, v in want.items() if f != "status"}
    rec, ops = sw_align_arrays(t, [0, 1], [0, 0], [q], ops_stride=1)  # the wrapper retries status 2 inside
    t.free()
    for p in range(2):
        _check(rec, ops, p, w, q)


# ------------------------------------------------------------------------------------------ mapper level
def test_reads_align_to_their_truth_windows():
    from deepreadmapper_amd import GenomeTable, extract_fasta_sequence, sam_cigar, sw_align_arrays, synth
    g = np.frombuffer(extract_fasta_sequence(os.path.join(GOLDEN, "ecoli_150.fna")), dtype=np.uint8).copy()
    reads, _, truth = synth.simulate_reads(g, 64, seed=31)
    q = [bytes(r) for r in synth.tag(reads)]
    t = GenomeTable(g, 150)
    rec, ops = sw_align_arrays(t, truth, np.arange(64), q)
    t.free()
    assert set(truth % 2) == {0, 1}
    for p in range(64):
        wid = int(truth[p])
        _check(rec, ops, p, R.window_bytes(g, 150, wid), q[p])
        pos1, cigar = sam_cigar(rec[p], ops[p], 152, 150, wid)
        assert (pos1, cigar) == R.sam_fields(rec[p], ops[p], 152, 150, wid)
        m = re.fullmatch(r"(?:(\d+)S)?(\d+)M(?:(\d+)S)?", cigar)  # substitutions only: 150M, or clipped ends
        assert m, cigar
        lead = int(m.group(1) or 0)
        assert lead + int(m.group(2)) + int(m.group(3) or 0) == 150
        # forward: the read starts at the truth position; reverse: the reversed CIGAR's leading clip is the read's
        # trailing one, which again sits at the window's leftmost base
        assert pos1 == wid // 2 + 1 + lead, (p, wid, cigar)


# ------------------------------------------------------------------------------------------ CLI
def test_pipeline_cli_sam_cigar(tmp_path):
    """test_pipeline_cli_dynamic_and_sam_streaming's recipe with DRM_SAM_CIGAR=1 (4 rows per read, so that the
    Python restatement of every row stays quick)."""
    from deepreadmapper_amd import extract_fasta_sequence
    fna = os.path.join(GOLDEN, "ecoli_150.fna")
    fq = os.path.join(GOLDEN, "test_data.fastq")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    r = subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), fna, "c1", "150"], cwd=tmp_path, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    base = [os.path.join(ROOT, "bin", "pipeline"), "c1", fq, fna, "128", "4", "4"]
    for name, extra, cigar in (("static", ["0", "0"], "0"), ("stream", ["1", "1"], "1")):
        e = dict(os.environ, DRM_SAM_BLOCK="40", DRM_SAM_CIGAR=cigar)  # several SAM blocks for 150 reads
        r = subprocess.run(base + [name] + extra, cwd=tmp_path, env=e, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    g = extract_fasta_sequence(fna)
    lines = open(fq, "rb").read().split(b"\n")
    recs = [(lines[i], lines[i + 1]) for i in range(0, len(lines) - 1, 4) if lines[i].startswith(b"@")]
    qids = [h[1:].split(b" ")[0].split(b"\t")[0].split(b"/")[0].decode() for h, _ in recs]
    ids = np.load(tmp_path / "static" / "indices.npy")
    assert ids.shape == (len(recs), 4)
    want = ["@HD\tVN:1.0\tSO:unsorted", "@SQ\tSN:ref\tLN:150"]
    mapped = 0
    for i, (_, read) in enumerate(recs):
        q = b"<" + read + b">"
        for j in range(4):
            wid = int(ids[i, j])
            rec, ops = R.align(R.window_bytes(g, 150, wid), q)
            flag = (0 if j == 0 else 256) | (16 if wid % 2 else 0)
            seq = (R.revcomp(read) if wid % 2 else read).decode()
            if rec["status"] == 1:
                want.append(f"{qids[i]}\t{flag | 4}\tref\t0\t60\t*\t*\t0\t0\t{seq}\t*")
                continue
            pos1, cigar = R.sam_fields(rec, ops, len(q), 150, wid)
            assert R.cigar_query_length(cigar) == len(seq)
            want.append(f"{qids[i]}\t{flag}\tref\t{pos1}\t60\t{cigar}\t*\t0\t0\t{seq}\t*\tAS:i:{rec['score']}\tNM:i:{rec['nm']}")
            mapped += 1
    assert mapped > len(recs)
    got = open(tmp_path / "stream" / "results.sam").read().split("\n")
    assert got[-1] == "" and got[:-1] == want
    # query shards on several devices (here the same one twice): the alignments run on a handle of their own
    e = dict(os.environ, DRM_SAM_BLOCK="40", DRM_SAM_CIGAR="1", DRM_DEVICES="0,0")
    r = subprocess.run(base + ["multi", "1", "1"], cwd=tmp_path, env=e, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(tmp_path / "multi" / "results.sam").read().split("\n") == got
    for line in got[2:-1]:
        f = line.split("\t")
        if f[5] != "*":
            assert R.cigar_query_length(f[5]) == len(f[9])


@pytest.mark.parametrize("rows", ["l2", "sw"])
def test_pipeline_cli_sam_cigar_sparse_rows(tmp_path, rows):
    """The other two branches that write rows, on a stride-2 index with DRM_SAM_L2_ROWS=1: the L2 rerank's rows
    (GRU model) and the SW rerank's rows (3-mer stand-in). The run without DRM_SAM_CIGAR names each row's window
    (POS = id / 2 + 1, flag 16 = odd id); the run with it must print that window's alignment on the same row."""
    from deepreadmapper_amd import extract_fasta_sequence
    from deepreadmapper_amd.encoder import DEFAULT_MODEL
    fna = os.path.join(GOLDEN, "ecoli_150.fna")
    fq = os.path.join(GOLDEN, "test_data.fastq")
    env = dict(os.environ, DRM_BUILD_THREADS="1", DRM_ENCODER=DEFAULT_MODEL if rows == "l2" else "kmer3",
               DRM_SAM_L2_ROWS="1", DRM_SAM_BLOCK="40")
    r = subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), fna, "s2", "150", "2"], cwd=tmp_path, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sams = {}
    for cigar in ("0", "1"):
        argv = [os.path.join(ROOT, "bin", "pipeline"), "s2", fq, fna, "128", "3", "64", "out" + cigar, "1", "1"]
        r = subprocess.run(argv, cwd=tmp_path, env=dict(env, DRM_SAM_CIGAR=cigar), capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("SAM rows from the SW rerank" in r.stdout) == (rows == "sw")
        sams[cigar] = open(tmp_path / ("out" + cigar) / "results.sam").read().split("\n")
    plain, real = sams["0"], sams["1"]
    assert len(plain) == len(real) > 50 and plain[:2] == real[:2] and plain[-1] == real[-1] == ""
    g = extract_fasta_sequence(fna)
    for a, b in zip(plain[2:-1], real[2:-1]):
        fa = a.split("\t")
        read = fa[9].encode()
        flag = int(fa[1])
        wid = 2 * (int(fa[3]) - 1) + (1 if flag & 16 else 0)
        q = b"<" + read + b">"
        rec, ops = R.align(R.window_bytes(g, 150, wid), q)
        seq = (R.revcomp(read) if wid % 2 else read).decode()
        if rec["status"] == 1:
            assert b == f"{fa[0]}\t{flag | 4}\tref\t0\t60\t*\t*\t0\t0\t{seq}\t*"
            continue
        pos1, cigar = R.sam_fields(rec, ops, len(q), 150, wid)
        assert b == f"{fa[0]}\t{flag}\tref\t{pos1}\t60\t{cigar}\t*\t0\t0\t{seq}\t*\tAS:i:{rec['score']}\tNM:i:{rec['nm']}"
        assert R.cigar_query_length(cigar) == len(seq)


# ------------------------------------------------------------------------------------------ limits, device form
def test_window_longer_than_256_is_unsupported():
    from deepreadmapper_amd import DrmError, sw_align_arrays
    from deepreadmapper_amd._native import DRM_ERR_UNSUPPORTED
    t = _table([b"ACGT" * 64 + b"A"])
    with pytest.raises(DrmError) as e:
        sw_align_arrays(t, [0], [0], [b"<ACGTACGT>"])
    t.free()
    assert e.value.code == DRM_ERR_UNSUPPORTED and "257" in str(e.value)


def test_device_entry_point_equals_host(short_pairs):
    from deepreadmapper_amd import sw_align_arrays
    from deepreadmapper_amd import rerank as RR
    from deepreadmapper_amd._native import check, lib
    from deepreadmapper_amd.device import DeviceBuffer, Stream
    windows, queries, _ = short_pairs
    combo = (37 * np.arange(300)) % 128
    wid, pq = (combo // 8).astype(np.uint64), (combo % 8).astype(np.int64)
    pq[7] = 8    # the device form cannot refuse a query index outside [0, nq): such a pair is status 1
    pq[11] = -1
    qbuf, qlen = RR.pack_queries(queries)
    t = _table(windows)
    st = Stream()
    d = [DeviceBuffer.from_host(x) for x in (wid, pq, qbuf, qlen)]
    d_rec, d_ops = DeviceBuffer(300, RR.SW_ALIGNMENT_DTYPE), DeviceBuffer((300, 16), np.uint32)
    d_ops.zero()
    check(lib().drm_sw_align_device(t.handle, d[0].ptr, d[1].ptr, 300, d[2].ptr, d[3].ptr, qbuf.shape[1], len(qlen),
                                    d_rec.ptr, d_ops.ptr, 16, st.handle))
    st.synchronize()
    rec, ops = d_rec.download(), d_ops.download()
    ok = np.ones(300, bool)
    ok[[7, 11]] = False
    want, wops = sw_align_arrays(t, wid[ok], pq[ok], queries)
    t.free()
    assert rec[ok].tobytes() == want.tobytes()
    assert [list(map(int, ops[p, :rec["n_ops"][p]])) for p in np.flatnonzero(ok)] == [list(map(int, o)) for o in wops]
    assert [tuple(int(x) for x in r) for r in rec[~ok]] == [(0, 0, 0, 0, 0, 0, 0, 1)] * 2
