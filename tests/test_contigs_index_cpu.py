"""CPU tests of bin/hnswpq_index under DRM_CONTIGS=1 (host builder, DRM_BUILD_DEVICE=cpu): the index of a multi-contig
FASTA holds every window of drm_extract_fasta_sequence's string, for a single-contig FASTA it is the index built
without the variable, and anything but a FASTA at stride 1 ends the run with "Error: ..." and exit code 1."""
import os
import subprocess

import numpy as np

import contig_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOOL = os.path.join(ROOT, "bin", "hnswpq_index")
REF_LEN = 30


def _run(cwd, args, contigs):
    env = dict(os.environ, DRM_BUILD_THREADS="1", DRM_BUILD_DEVICE="cpu", DRM_ENCODER="kmer3")
    env.pop("DRM_CONTIGS", None)
    if contigs:
        env["DRM_CONTIGS"] = "1"
    return subprocess.run([TOOL] + [str(a) for a in args], cwd=cwd, env=env, capture_output=True, text=True)


def _config(path):
    return dict(line.split(": ", 1) for line in open(path).read().splitlines())


def _three(tmp_path):
    rng = np.random.default_rng(3)
    seq = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))  # noqa: E731
    data = b">c1\n" + seq(400) + b"\n>c2 GATTACA cat\n" + seq(60) + b"\n>c3 tagged\n" + seq(250) + b"\n"
    (tmp_path / "three.fa").write_bytes(data)
    return data


def test_multi_contig_index_holds_every_window_of_the_genome_string(tmp_path):
    data = _three(tmp_path)
    g = R.extract(data)
    names, starts, lens = R.fasta_contigs(data)
    r = _run(tmp_path, ["three.fa", "ix", REF_LEN], True)
    assert r.returncode == 0, r.stderr
    nw = len(g) - REF_LEN + 1
    cfg = _config(tmp_path / "ix" / "config.txt")
    assert int(cfg["n_vects"]) == 2 * nw and int(cfg["stride"]) == 1 and int(cfg["ref_len"]) == REF_LEN
    inside = sum(max(int(n) - REF_LEN + 1, 0) for n in lens)
    assert f"{len(names)} contigs, {int(lens.sum())} bases" in r.stdout
    assert f"{nw - inside} of {nw} window positions" in r.stdout and 0 < inside < nw
    # window w of the index is g[w >> 1 : (w >> 1) + ref_len]: the index of a one-line FASTA of g, built the old way,
    # is the same file
    (tmp_path / "flat.fa").write_bytes(b">g\n" + g + b"\n")
    flat = _run(tmp_path, ["flat.fa", "flat", REF_LEN], False)
    assert flat.returncode == 0, flat.stderr
    assert (tmp_path / "ix" / "ix.index").read_bytes() == (tmp_path / "flat" / "flat.index").read_bytes()
    # without the variable the windows are cut per contig: fewer vectors, and ids that are no positions
    plain = _run(tmp_path, ["three.fa", "plain", REF_LEN], False)
    assert plain.returncode == 0, plain.stderr
    pcfg = _config(tmp_path / "plain" / "config.txt")
    assert int(pcfg["n_vects"]) == 2 * inside
    assert sorted(cfg) == sorted(pcfg)  # config.txt keeps its keys


def test_single_contig_index_is_the_one_built_today(tmp_path):
    # the fixture's header, "> Fake DNA sequence", has an empty name, which the contig table refuses: give it one
    body = open(os.path.join(GOLDEN, "ecoli_150.fna"), "rb").read().split(b"\n", 1)[1]
    fna = tmp_path / "ecoli.fna"
    fna.write_bytes(b">ecoli Fake DNA sequence\n" + body)
    a = _run(tmp_path, [fna, "with", 150], True)
    b = _run(tmp_path, [fna, "without", 150], False)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert "1 contigs" in a.stdout and "0 of 851 window positions" in a.stdout
    assert (tmp_path / "with" / "with.index").read_bytes() == (tmp_path / "without" / "without.index").read_bytes()


def test_requirements(tmp_path):
    _three(tmp_path)
    (tmp_path / "w.txt").write_bytes(b"ACGT" * 10 + b"\n")
    np.save(tmp_path / "e.npy", np.zeros((4, 128), np.float32))
    for args in (["three.fa", "a", REF_LEN, 2], ["w.txt", "b", REF_LEN], ["e.npy", "c", REF_LEN]):
        r = _run(tmp_path, args, True)
        assert r.returncode == 1 and r.stderr.startswith("Error: ") and "DRM_CONTIGS" in r.stderr, (args, r.stderr)
        assert not (tmp_path / args[1]).exists()
    (tmp_path / "iupac.fa").write_bytes(b">a\nACGTACGTRACGT\n")
    r = _run(tmp_path, ["iupac.fa", "d", 4], True)
    assert r.returncode == 1 and r.stderr.startswith("Error: ") and '"a"' in r.stderr
