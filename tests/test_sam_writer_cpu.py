"""The SAM writers (write_sam_block / write_sam_pairs, deepreadmapper_amd/csrc/sam.cpp) on the CPU:
tests/sam_writer_driver.cpp builds small blocks in code -- pseudo rows, aligned rows in window and region mode, MD, contigs, lines per locus and
XA, pairs, pairs on two contigs, pairs with XA, the writers' own errors -- and writes one file per case, which must
equal tests/golden/sam_writer/<case>.sam byte for byte. The golden files are this writer's own output, recorded before
it was restructured; a change to them is a change to the SAM text. The driver and the writer's source are compiled
with AddressSanitizer and UBSan into a plain executable: nothing is preloaded and no GPU is needed.

`flush` is one block of 40000 aligned reads (15 MB, past the writer's 4 MiB flush three times); its golden file holds
only the byte count and the SHA-256.

To record again after a deliberate change of the text: run the driver into a directory and copy its files, writing
`digest()` of flush.sam in place of the file."""
import hashlib
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "deepreadmapper_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sam_writer")
DIGESTS = {"flush"}  # cases kept as "<bytes> <sha256>\n"
CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".sam"))
WRITER = os.path.join(CSRC, "sam.cpp")  # the writer's whole translation unit


def digest(path):
    with open(path, "rb") as f:
        data = f.read()
    return f"{len(data)} {hashlib.sha256(data).hexdigest()}\n".encode()


@pytest.fixture(scope="module")
def produced(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_writer")
    exe = str(d / "sam_writer_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-D__HIP_PLATFORM_AMD__",
                    "-I/opt/rocm/include", "-fopenmp", WRITER, os.path.join(ROOT, "tests", "sam_writer_driver.cpp"),
                    "-o", exe], check=True)
    out = d / "out"
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr  # a sanitizer report goes to stderr
    return out


def test_every_case_is_recorded():
    assert {"pseudo", "pseudo_mapq", "aligned", "region", "md", "contigs", "loci", "loci_xa", "loci_plain",
            "loci_xa_plain", "pairs", "pairs_mapq", "pairs_contigs", "pairs_xa", "pairs_xa_plain", "flush",
            "errors"} == set(CASES)


DUP_READS = {"r0", "S1/3/0", "r4"}  # the driver's loci_dup: reads 0, 2 and 4 (reads 2 and 5 have no id of their own)
DUP_PAIRS = {"p0", "p2", "S1/6/0"}  # pairs_dup: pairs 0, 2 and 5


@pytest.mark.parametrize("case,base,names", [("loci_dup", "loci", DUP_READS), ("pairs_dup", "pairs", DUP_PAIRS)])
def test_dup_adds_1024_to_every_line_of_the_chosen_reads(produced, case, base, names):
    """The per-read `dup` field of a block: the file is the base case's recorded file with 1024 added to the flag of
    every line -- primary, secondary, unmapped, both mates -- of the chosen reads, and nothing else changes."""
    with open(os.path.join(GOLDEN, base + ".sam")) as f:
        recorded = f.read().split("\n")
    want, marked = [], set()
    for line in recorded:
        f = line.split("\t")
        if not line.startswith("@") and f[0] in names:
            assert not int(f[1]) & 1024
            f[1] = str(int(f[1]) + 1024)
            marked.add(f[0])
        want.append("\t".join(f))
    assert marked == names and any(int(x.split("\t")[1]) & 4 for x in want if x.split("\t")[0] in names)
    assert (produced / (case + ".sam")).read_text().split("\n") == want


@pytest.mark.parametrize("case", CASES)
def test_sam_text_is_the_recorded_one(produced, case):
    path = produced / (case + ".sam")
    with open(os.path.join(GOLDEN, case + ".sam"), "rb") as f:
        want = f.read()
    got = digest(path) if case in DIGESTS else path.read_bytes()
    assert got == want, f"{case}: the writer's text differs from tests/golden/sam_writer/{case}.sam"
