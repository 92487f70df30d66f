"""CPU tests of the boundary: the C-ABI library loads and exports every symbol include/drm_hip.h
declares; host-only entry points (index build, embedder, argument validation) work without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, "include", "drm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(drm_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from deepreadmapper_amd import _native
    lib = _native.lib()
    declared = _declared()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), name
    assert sorted(_native.EXPORTS) == declared


def test_nm_exports_are_plain_c():
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "deepreadmapper_amd", "libdrm_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in _declared():
        assert name in syms, name  # unmangled extern "C"


def test_embedder_deterministic_and_normalised():
    from deepreadmapper_amd import synth
    a = synth.embed([b"<ACGTACGTAC>", b"NNNN", b"ACGTTGCA"])
    b = synth.embed([b"ACGTACGTAC", b"NNNN", b"ACGTTGCA"])
    assert np.array_equal(a, b)  # tags are not ACGT 3-mers
    assert abs(np.linalg.norm(a[0]) - 1) < 1e-5 and not a[1].any()


def test_build_and_reader_roundtrip(tmp_path):
    from deepreadmapper_amd import synth
    from oracle import faiss_file
    rng = np.random.default_rng(1)
    x = rng.standard_normal((600, 32)).astype(np.float32)
    p1, p2 = str(tmp_path / "a.index"), str(tmp_path / "b.index")
    synth.build_index(x, p1, M_pq=4, nbits=8, M_hnsw=8, efc=40, nthreads=1, seed=3)
    synth.build_index(x, p2, M_pq=4, nbits=8, M_hnsw=8, efc=40, nthreads=1, seed=3)
    assert open(p1, "rb").read() == open(p2, "rb").read()  # single-threaded build is deterministic
    fx = faiss_file.read(p1)
    assert fx.d == 32 and fx.ntotal == 600 and fx.pq_M == 4 and fx.pq_nbits == 8
    assert len(fx.offsets) == 601 and fx.offsets[-1] == len(fx.neighbors)
    assert fx.cum_nneighbor_per_level[1] == 16 and fx.codes.size == 600 * 4
    assert fx.levels[fx.entry_point] == fx.max_level + 1
    assert ((fx.neighbors >= -1) & (fx.neighbors < 600)).all()


def test_build_rejects_bad_args(tmp_path):
    from deepreadmapper_amd import synth, DrmError
    with pytest.raises(DrmError):
        synth.build_index(np.zeros((10, 30), np.float32), str(tmp_path / "x.index"), M_pq=8)


def test_index_load_rejects_non_hnswpq(tmp_path):
    from deepreadmapper_amd import read_index, DrmError
    from deepreadmapper_amd._native import DRM_ERR_FORMAT, DRM_ERR_IO
    bad = tmp_path / "bad.index"
    bad.write_bytes(b"IHNf" + b"\0" * 64)
    with pytest.raises(DrmError) as e:
        read_index(str(bad))
    assert e.value.code == DRM_ERR_FORMAT and "IHNf" in str(e.value)
    with pytest.raises(DrmError) as e:
        read_index(str(tmp_path / "missing.index"))
    assert e.value.code == DRM_ERR_IO


def test_index_load_rejects_truncated(tmp_path, c1):
    from deepreadmapper_amd import read_index, DrmError
    from deepreadmapper_amd._native import DRM_ERR_FORMAT
    data = open(c1["index"], "rb").read()
    t = tmp_path / "trunc.index"
    t.write_bytes(data[: len(data) // 2])
    with pytest.raises(DrmError) as e:
        read_index(str(t))
    assert e.value.code == DRM_ERR_FORMAT and "truncated" in str(e.value)


def test_hnswpq_index_cli(tmp_path):
    """bin/hnswpq_index mirrors src/hnswpq/index.cpp:195-316: config.txt keys + prefix/prefix.index."""
    exe = os.path.join(ROOT, "bin", "hnswpq_index")
    fna = os.path.join(ROOT, "tests", "golden", "ecoli_150.fna")
    env = dict(os.environ, DRM_BUILD_THREADS="1")
    r = subprocess.run([exe, fna, "c1idx", "150"], cwd=tmp_path, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    cfg = dict(l.split(": ", 1) for l in (tmp_path / "c1idx" / "config.txt").read_text().splitlines())
    assert cfg == {"index_type": "HNSWPQ", "stride": "1", "ref_len": "150", "n_vects": "1702", "dim": "128",
                   "M_hnsw": "16", "EFC": "200", "M_pq": "8", "nbits": "8", "index_file": "c1idx/c1idx.index"}
    from oracle import faiss_file
    fx = faiss_file.read(str(tmp_path / "c1idx" / "c1idx.index"))
    assert fx.ntotal == 1702
    r = subprocess.run([exe, fna], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stderr


def test_index_load_rejects_upper_link_to_lower_node(tmp_path, c1):
    """A level-l link must target a node that reaches level l (faiss IHNp): the kernel would read
    the target's level-l list, which does not exist. Rejected as DRM_ERR_FORMAT before any GPU use."""
    from deepreadmapper_amd import read_index, DrmError
    from deepreadmapper_amd._native import DRM_ERR_FORMAT
    fx = c1["fx"]
    lv, cum, offs = fx.levels, fx.cum_nneighbor_per_level, fx.offsets
    pos = 4 + 33 + (8 + 8 * len(fx.assign_probas)) + (8 + 4 * len(cum)) + (8 + 4 * len(lv)) + (8 + 8 * len(offs)) + 8
    src = int(np.flatnonzero(lv >= 2)[0])
    low = int(np.flatnonzero(lv == 1)[0])
    slot = int(offs[src]) + int(cum[1])  # first level-1 link of src
    data = bytearray(open(c1["index"], "rb").read())
    data[pos + 4 * slot: pos + 4 * slot + 4] = np.int32(low).tobytes()
    bad = tmp_path / "uplink.index"
    bad.write_bytes(bytes(data))
    with pytest.raises(DrmError) as e:
        read_index(str(bad))
    assert e.value.code == DRM_ERR_FORMAT and "does not reach" in str(e.value)


def test_flat_index_load_rejects_upper_link_to_lower_node(tmp_path):
    """Same check on the hnswlib reader (an upper link to a level-0 element)."""
    from deepreadmapper_amd import synth, DrmError
    from deepreadmapper_amd.flat import HnswFlatIndex
    from deepreadmapper_amd._native import DRM_ERR_FORMAT
    from oracle import hnswlib_file
    rng = np.random.default_rng(0)
    x = rng.standard_normal((3000, 16)).astype(np.float32)
    path = str(tmp_path / "f.hnsw")
    synth.build_flat_index(x, path, M=8, efc=32, nthreads=1)
    fx = hnswlib_file.read(path)
    n, maxM0, maxM, d = fx["n"], fx["maxM0"], fx["maxM"], fx["d"]
    sz_el = 4 * (1 + maxM0) + 4 * d + 8
    pos = 96 + n * sz_el
    low = int(np.flatnonzero(fx["levels"] == 0)[0])
    data = bytearray(open(path, "rb").read())
    for i in range(n):
        size = int(np.frombuffer(data[pos:pos + 4], np.uint32)[0])
        pos += 4
        if size and int(np.frombuffer(data[pos:pos + 4], np.uint32)[0]) & 0xFFFF:
            data[pos + 4:pos + 8] = np.uint32(low).tobytes()  # first level-1 link
            break
        pos += size
    bad = tmp_path / "bad.hnsw"
    bad.write_bytes(bytes(data))
    with pytest.raises(DrmError) as e:
        HnswFlatIndex(str(bad))
    assert e.value.code == DRM_ERR_FORMAT and "does not reach" in str(e.value)


def test_pipeline_rejects_ragged_reference(tmp_path):
    """a .txt reference with a line shorter than ref_len is refused with a format
    error before the GPU is touched (the fixed-width window table would over-read it)."""
    exe = os.path.join(ROOT, "bin", "pipeline")
    prefix = tmp_path / "idx"
    prefix.mkdir()
    (prefix / "config.txt").write_text("ref_len: 150\nstride: 1\n")
    (prefix / "idx.index").write_bytes(b"")
    ref = tmp_path / "ref.txt"
    ref.write_text("A" * 150 + "\n" + "C" * 149 + "\n")
    q = tmp_path / "q.txt"
    q.write_text("A" * 150 + "\n")
    r = subprocess.run([exe, str(prefix), str(q), str(ref)], capture_output=True, text=True)
    assert r.returncode == 1 and "reference sequence 1 has 149 bytes" in r.stderr


# bin/pipeline's option checks, all of which run before the index or a device is touched: the environment on top of
# DRM_SAM_CIGAR=1 (None = unset), the argv positions replaced in `pipeline idx m1.fastq g.fna 128 4 4 out 1 1`, and the
# text after "Error: " that the binary printed before the options moved into one record (tools/pipeline.cpp)
_MATES = {"DRM_MATES": "m2.fastq"}
_RESCUE = {**_MATES, "DRM_PAIR_RESCUE": "1"}
_MAPQ = {"DRM_SAM_MAPQ": "1"}
_SCORING_RANGES = ("DRM_SAM_SCORING must be match,mismatch,open,extend with match 1..31, mismatch 1..63, open 0..63, "
                   "extend 1..63: ")
_NEEDS_STREAM = "DRM_MATES needs use_dynamic=1 and use_streaming=1: pairs are written to the streamed SAM"
_MATES_ONE_DEVICE = "DRM_MATES runs on one device (DRM_DEVICE), not on DRM_DEVICES"
_BAD_OPTIONS = [
    ("scoring_three", {"DRM_SAM_SCORING": "1,4,6"}, {}, _SCORING_RANGES + '"1,4,6"'),
    ("scoring_token", {"DRM_SAM_SCORING": "1,4,x,1"}, {},
     'DRM_SAM_SCORING must be match,mismatch,open,extend (four non-negative integers): "1,4,x,1"'),
    ("scoring_range", {"DRM_SAM_SCORING": "0,4,6,1"}, {}, _SCORING_RANGES + '"0,4,6,1"'),
    ("flank_negative", {"DRM_SAM_FLANK": "-1"}, {}, 'DRM_SAM_FLANK must be a non-negative integer: "-1"'),
    ("flank_wide", {"DRM_SAM_FLANK": "54"}, {}, "DRM_SAM_FLANK 54: ref_len 150 + 2 * flank > 256"),
    ("tlen_one", {**_MATES, "DRM_PAIR_TLEN": "100"}, {},
     'DRM_PAIR_TLEN must be min,max (two non-negative integers): "100"'),
    ("tlen_order", {**_MATES, "DRM_PAIR_TLEN": "500,100"}, {},
     'DRM_PAIR_TLEN must be min,max with 0 <= min <= max <= 2^30: "500,100"'),
    ("tlen_token", {**_MATES, "DRM_PAIR_TLEN": "0,1e3"}, {},
     'DRM_PAIR_TLEN must be min,max (two non-negative integers): "0,1e3"'),
    ("penalty_negative", {**_MATES, "DRM_PAIR_PENALTY": "-1"}, {},
     'DRM_PAIR_PENALTY must be an integer in [0, 2^20]: "-1"'),
    ("pairs_not_streaming", _MATES, {9: "0"}, _NEEDS_STREAM),
    ("pairs_not_dynamic", _MATES, {8: "0"}, _NEEDS_STREAM),
    ("pairs_no_cigar", {**_MATES, "DRM_SAM_CIGAR": None}, {},
     "DRM_MATES needs DRM_SAM_CIGAR=1: the pair fields come from real alignments"),
    ("mates_missing", {"DRM_MATES": "missing.fastq"}, {}, "Could not open file: missing.fastq"),
    ("mates_empty", {"DRM_MATES": ""}, {}, "DRM_MATES is empty: it names the file of second mates"),
    ("mates_short", {"DRM_MATES": "m2short.fastq"}, {},
     "DRM_MATES: m1.fastq has 2 records and m2short.fastq has 1: record 1 has no mate"),
    ("mates_renamed", {"DRM_MATES": "m2renamed.fastq"}, {},
     'DRM_MATES: record 1 is named "r1" in m1.fastq and "x1" in m2renamed.fastq'),
    ("pairs_two_devices", {**_MATES, "DRM_DEVICES": "0,0"}, {}, _MATES_ONE_DEVICE),
    ("rescue_min_negative", {**_RESCUE, "DRM_PAIR_RESCUE_MIN": "-1"}, {},
     'DRM_PAIR_RESCUE_MIN must be an integer in [0, 2^20]: "-1"'),
    ("rescue_min_token", {**_RESCUE, "DRM_PAIR_RESCUE_MIN": "4x"}, {},
     'DRM_PAIR_RESCUE_MIN must be an integer in [0, 2^20]: "4x"'),
    ("rescue_min_empty", {**_RESCUE, "DRM_PAIR_RESCUE_MIN": ""}, {},
     'DRM_PAIR_RESCUE_MIN must be an integer in [0, 2^20]: ""'),
    ("rescue_min_large", {**_RESCUE, "DRM_PAIR_RESCUE_MIN": "1048577"}, {},
     'DRM_PAIR_RESCUE_MIN must be an integer in [0, 2^20]: "1048577"'),
    ("rescue_window", {**_RESCUE, "DRM_PAIR_TLEN": "0,5000"}, {},
     "template lengths [0, 5000] at ref_len 150 give a rescue region of 5000 > 2048 rows"),
    ("mapq_min_negative", {**_MAPQ, "DRM_MAPQ_MIN": "-1"}, {}, 'DRM_MAPQ_MIN must be an integer in [0, 2^20]: "-1"'),
    ("mapq_min_negative_pairs", {**_MAPQ, **_MATES, "DRM_MAPQ_MIN": "-1"}, {},
     'DRM_MAPQ_MIN must be an integer in [0, 2^20]: "-1"'),
    ("mapq_min_token", {**_MAPQ, "DRM_MAPQ_MIN": "4x"}, {}, 'DRM_MAPQ_MIN must be an integer in [0, 2^20]: "4x"'),
    ("mapq_min_empty", {**_MAPQ, "DRM_MAPQ_MIN": ""}, {}, 'DRM_MAPQ_MIN must be an integer in [0, 2^20]: ""'),
    ("mapq_min_large", {**_MAPQ, "DRM_MAPQ_MIN": "1048577"}, {},
     'DRM_MAPQ_MIN must be an integer in [0, 2^20]: "1048577"'),
    ("mapq_span_zero", {**_MAPQ, "DRM_MAPQ_SPAN": "0"}, {}, 'DRM_MAPQ_SPAN must be an integer in [1, 2^20]: "0"'),
    ("mapq_span_zero_pairs", {**_MAPQ, **_MATES, "DRM_MAPQ_SPAN": "0"}, {},
     'DRM_MAPQ_SPAN must be an integer in [1, 2^20]: "0"'),
    ("mapq_span_token", {**_MAPQ, "DRM_MAPQ_SPAN": "1e2"}, {}, 'DRM_MAPQ_SPAN must be an integer in [1, 2^20]: "1e2"'),
    ("mapq_span_large", {**_MAPQ, "DRM_MAPQ_SPAN": "1048577"}, {},
     'DRM_MAPQ_SPAN must be an integer in [1, 2^20]: "1048577"'),
    ("mapq_two_devices", {**_MAPQ, "DRM_DEVICES": "0,0"}, {},
     "DRM_SAM_MAPQ runs on one device (DRM_DEVICE), not on DRM_DEVICES"),
    ("mapq_two_devices_pairs", {**_MAPQ, **_MATES, "DRM_DEVICES": "0,0"}, {}, _MATES_ONE_DEVICE),
    ("mapq_l2_rows", {**_MAPQ, "DRM_SAM_L2_ROWS": "1"}, {},
     "DRM_SAM_MAPQ does not go with DRM_SAM_L2_ROWS=1: those rows carry distances, not scores"),
]


@pytest.fixture(scope="module")
def option_dir(tmp_path_factory):
    """A prefix directory with nothing but config.txt, and four-base FASTQ files: enough for every option check."""
    d = tmp_path_factory.mktemp("options")
    (d / "idx").mkdir()
    (d / "idx" / "config.txt").write_text("ref_len: 150\nstride: 1\n")

    def fastq(names):
        return "".join(f"@{n}\n{s}\n+\nIIII\n" for n, s in zip(names, ("ACGT", "TTGA")))
    (d / "m1.fastq").write_text(fastq(("r0", "r1")))
    (d / "m2.fastq").write_text(fastq(("r0", "r1")))
    (d / "m2short.fastq").write_text(fastq(("r0",)))
    (d / "m2renamed.fastq").write_text(fastq(("r0", "x1")))
    return d


@pytest.mark.parametrize("env,argv,message", [c[1:] for c in _BAD_OPTIONS], ids=[c[0] for c in _BAD_OPTIONS])
def test_pipeline_rejects_bad_options(option_dir, env, argv, message):
    """Every fault in argv or a DRM_* variable ends the run with exit status 1 and the same text as before, ahead of
    the index load (which the directory could not serve)."""
    args = [os.path.join(ROOT, "bin", "pipeline"), "idx", "m1.fastq", "g.fna", "128", "4", "4", "out", "1", "1"]
    for i, v in argv.items():
        args[i] = v
    e = {k: v for k, v in os.environ.items() if not k.startswith("DRM_")}
    e.update({k: v for k, v in {"DRM_SAM_CIGAR": "1", **env}.items() if v is not None})
    r = subprocess.run(args, cwd=option_dir, env=e, capture_output=True, text=True)
    assert r.returncode == 1
    assert r.stderr == "Error: " + message + "\n"
    assert "Index loaded" not in r.stdout
