"""The spool and the final writer of DRM_SAM_SORT=coordinate (SamSpool, write_sam_sorted, deepreadmapper_amd/csrc/sam.cpp)
on the CPU: tests/sam_sort_driver.cpp writes sam_writer_driver.cpp's blocks once as they are and once through a spool,
a std::stable_sort of the spool's keys and the final writer. The unsorted file is the recorded one of
tests/golden/sam_writer where there is one; the sorted file is the unsorted one with @HD replaced and the body put through
Python's stable sorted() under (RNAME == "*", index of RNAME among the @SQ lines, POS, flag & 16), byte for byte; the
spooled key of every line is therefore drm_sam_sort_key of those columns. What the final writer refuses leaves no file.
The writer's source and the driver are compiled with AddressSanitizer and UBSan into a plain executable: nothing is
preloaded and no GPU is needed."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "deepreadmapper_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "sam_writer")
CASES = ["aligned", "contigs", "loci", "loci_dup", "loci_xa", "pairs", "pairs_dup", "pairs_contigs", "pairs_xa", "flush"]
RECORDED = ["aligned", "contigs", "loci", "loci_xa", "pairs", "pairs_contigs", "pairs_xa"]


@pytest.fixture(scope="module")
def produced(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_sort")
    exe = str(d / "sam_sort_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"),
                    "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fopenmp", os.path.join(CSRC, "sam.cpp"),
                    os.path.join(ROOT, "tests", "sam_sort_driver.cpp"), "-o", exe], check=True)
    out = d / "out"
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr  # a sanitizer report goes to stderr
    return out


def _lines(path):
    got = open(path).read().split("\n")
    assert got[-1] == ""
    return got[:-1]


def _by_python(lines):
    head = [x for x in lines if x.startswith("@")]
    body = lines[len(head):]
    assert head[0] == "@HD\tVN:1.0\tSO:unsorted" and not any(x.startswith("@") for x in body)
    names = [x.split("\t")[1][3:] for x in head[1:]]

    def key(line):
        f = line.split("\t")
        return (f[2] == "*", 0 if f[2] == "*" else names.index(f[2]), int(f[3]), int(f[1]) & 16)
    return ["@HD\tVN:1.0\tSO:coordinate"] + head[1:] + sorted(body, key=key), [key(x) for x in body]


@pytest.mark.parametrize("case", CASES)
def test_sorted_file_is_the_unsorted_file_sorted(produced, case):
    unsorted = _lines(produced / (case + ".unsorted.sam"))
    if case in RECORDED:
        assert unsorted == _lines(os.path.join(GOLDEN, case + ".sam"))
    want, keys = _by_python(unsorted)
    assert _lines(produced / (case + ".sorted.sam")) == want
    assert keys != sorted(keys), "the case is in coordinate order already"
    if case == "flush":
        assert len(keys) == 40000 and len(set(keys)) < len(keys) and len({k[1] for k in keys}) == 2


def test_the_cases_hold_equal_keys_lines_without_rname_and_unmapped_mates_beside_their_mates(produced):
    seen = {"equal": 0, "star": 0, "beside": 0}
    for case in CASES:
        unsorted = _lines(produced / (case + ".unsorted.sam"))
        keys = _by_python(unsorted)[1]
        seen["equal"] += len(set(keys)) < len(keys)
        seen["star"] += any(k[0] for k in keys)
        seen["beside"] += any(int(f[1]) & 4 and f[2] != "*" and int(f[3]) > 0
                              for f in (x.split("\t") for x in unsorted if not x.startswith("@")))
    assert all(seen.values()), seen


def test_the_small_spools_and_the_refused_ones(produced):
    assert open(produced / "two_lines.sorted.sam").read() == "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:ref\tLN:12\nb\na\n"
    assert open(produced / "empty.sorted.sam").read() == "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:ref\tLN:12\n"
    left = sorted(os.listdir(produced))
    assert not [x for x in left if x.startswith("err_") or x.endswith(".part")], left
