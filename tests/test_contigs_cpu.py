"""CPU tests of the multi-contig host side (include/drm_hip.h): drm_fasta_contigs against the plain restatement of
tests/contig_ref.py and against drm_extract_fasta_sequence's string, its format errors, the host lookup
drm_contigs_find at every boundary, and the argument errors of drm_contigs_create. No device is needed: a table is
copied to its device only by the first contig stage that runs."""
import numpy as np
import pytest

import contig_ref as R

REF_LEN = 10

ONE = b">chr1 the only one\nACGTACGTAC\nGGTTAACC\n"
THREE = (b">chrA first\nACGTACGTACGTAAC\nGGCCTTAGA\n"
         b">chrB GATTACA cat\nTTGACCAGTA\nCCA\n"
         b">chrC\ttagged NNN\nACGTNNACGTACGGT\n")
FASTAS = {
    "one": ONE,
    "three": THREE,
    "lower": b">a x\nacgtacgtacgt\nnnacgt\n>b acgt\nggccaattggcc\n",
    "crlf": THREE.replace(b"\n", b"\r\n"),
    "blank": b">a\n\nACGTACGTACGT\n\n\n>b tag\n\nGGCCAATTGGCC\n  \n",
    "no_newline": b">a\nACGTACGTACGT\n>b CAT\nGGCCAATTGGCC",
    "short": b">long\nACGTACGTACGTACGTACGT\n>tiny A\nACGTA\n>long2\nGGCCAATTGGCCAATT\n",
}


def _write(tmp_path, name, data):
    p = tmp_path / f"{name}.fa"
    p.write_bytes(data)
    return str(p)


@pytest.mark.parametrize("name", sorted(FASTAS))
def test_fasta_contigs_equal_the_restatement_and_slice_the_genome_string(tmp_path, name):
    from deepreadmapper_amd import extract_fasta_sequence, fasta_contigs
    data = FASTAS[name]
    path = _write(tmp_path, name, data)
    names, starts, lens = fasta_contigs(path)
    wn, ws, wl = R.fasta_contigs(data)
    assert names == wn and np.array_equal(starts, ws) and np.array_equal(lens, wl)
    assert starts.dtype == np.int64 and lens.dtype == np.int64
    g = extract_fasta_sequence(path)
    assert g == R.extract(data)
    # the invariant: g[start : start + len] is the contig's own sequence, the table ascending and disjoint
    seqs, cur = [], None
    for line in data.split(b"\n"):
        if line.startswith(b">"):
            cur = []
            seqs.append(cur)
        else:
            cur.append(bytes(c for c in line.upper() if c in R.BASES))
    assert len(seqs) == len(names)
    for t in range(len(names)):
        assert g[starts[t]:starts[t] + lens[t]] == b"".join(seqs[t])
        assert lens[t] >= 1 and (t == 0 or starts[t] >= starts[t - 1] + lens[t - 1])
    assert starts[0] == 0 and starts[-1] + lens[-1] == len(g)


def test_header_letters_are_gaps_and_a_short_contig_is_kept(tmp_path):
    from deepreadmapper_amd import fasta_contigs
    names, starts, lens = fasta_contigs(_write(tmp_path, "three", THREE))
    assert names == ["chrA", "chrB", "chrC"]
    # ">chrB GATTACA cat" holds c, G, A, T, T, A, C, A, c, a, t = 11 letters; ">chrC\ttagged NNN": c, C, t, a, g, g, N, N, N
    assert starts.tolist() == [0, 24 + 11, 24 + 11 + 13 + 9] and lens.tolist() == [24, 13, 15]
    names, starts, lens = fasta_contigs(_write(tmp_path, "short", FASTAS["short"]))
    assert names == ["long", "tiny", "long2"] and lens.tolist() == [20, 5, 16] and lens[1] < REF_LEN


@pytest.mark.parametrize("data,contig,word", [
    (b"ACGT\n>a\nACGT\n", 0, "contig 0"),                     # a first line without '>'
    (b"", 0, "contig 0"),
    (b">a\nACGT\n> spaced\nACGT\n", 1, "contig 1"),            # an empty name
    (b">a\nACGT\n>b\nACGT\n>a again\nACGT\n", 2, '"a"'),      # a duplicate name
    (b">a\nACGT\n>b\n>c\nACGT\n", 1, '"b"'),                   # a contig of length 0
    (b">a\nACGT\n>b\n", 1, '"b"'),                             # ... at the end of the file
    (b">a\n", 0, '"a"'),
    (b">a\nACGT\n>chrY\nACGRT\n", 1, '"chrY"'),                # a sequence byte the extraction drops
    (b">chrX\nAC-GT\n", 0, '"chrX"'),
])
def test_format_errors_name_the_contig(tmp_path, data, contig, word):
    from deepreadmapper_amd import DrmError, fasta_contigs
    from deepreadmapper_amd._native import DRM_ERR_FORMAT
    with pytest.raises(R.FormatError) as want:
        R.fasta_contigs(data)
    assert want.value.contig == contig
    with pytest.raises(DrmError) as e:
        fasta_contigs(_write(tmp_path, "bad", data))
    assert e.value.code == DRM_ERR_FORMAT
    assert word in str(e.value) and f"contig {contig}" in str(e.value)


def test_a_missing_file_is_an_io_error(tmp_path):
    from deepreadmapper_amd import DrmError, fasta_contigs
    from deepreadmapper_amd._native import DRM_ERR_IO
    with pytest.raises(DrmError) as e:
        fasta_contigs(str(tmp_path / "nothing.fa"))
    assert e.value.code == DRM_ERR_IO


def test_find_at_every_boundary():
    from deepreadmapper_amd import ContigTable
    # contigs [0, 30), [40, 50) (exactly REF_LEN), [55, 60) (shorter than REF_LEN), [60, 100) (no gap in front)
    starts, lens = [0, 40, 55, 60], [30, 10, 5, 40]
    t = ContigTable(starts, lens)
    cases = [(20, REF_LEN, 0), (21, REF_LEN, -1),          # ends at the contig's end / one base beyond
             (0, REF_LEN, 0), (40, REF_LEN, 1), (39, REF_LEN, -1), (41, REF_LEN, -1),  # at the start / one before
             (32, REF_LEN, -1), (30, 1, -1), (35, 0, -1),  # inside a gap
             (55, REF_LEN, -1), (55, 5, 2), (55, 6, -1),   # a contig shorter than the window
             (59, 1, 2), (60, 1, 3), (58, 4, -1),          # adjoining contigs: a window across their seam
             (90, REF_LEN, 3), (91, REF_LEN, -1), (100, 0, 3), (101, 0, -1), (100, REF_LEN, -1), (10**12, REF_LEN, -1),
             (2**62, REF_LEN, -1), (2**63 - 1, REF_LEN, -1), (2**63 - 1, 2**63 - 1, -1),
             (-1, REF_LEN, -1), (5, -1, -1), (0, 0, 0), (29, 1, 0), (0, 30, 0), (0, 31, -1)]
    for pos, span, want in cases:
        assert R.find(starts, lens, pos, span) == want, (pos, span)
        assert t.find(pos, span) == want, (pos, span)
    for pos in range(-2, 104):
        for span in (0, 1, 5, REF_LEN):
            assert t.find(pos, span) == R.find(starts, lens, pos, span), (pos, span)
    assert len(t) == 4
    t.free()
    t.free()  # a second free is harmless


@pytest.mark.parametrize("starts,lens", [
    ([], []),                                  # no contig
    ([0, 10], [10, 0]),                        # a length below 1
    ([0, 10], [11, 5]),                        # overlapping
    ([10, 0], [5, 5]),                         # descending
    ([-1], [5]),
    ([0], [2**40 + 1]),                        # an end beyond 2^40
    ([2**40], [1]),
    ([2**62], [2**62]),                        # a sum that would wrap
])
def test_create_rejects_a_bad_table(starts, lens):
    from deepreadmapper_amd import ContigTable, DrmError
    from deepreadmapper_amd._native import DRM_ERR_ARG
    with pytest.raises(DrmError) as e:
        ContigTable(starts, lens)
    assert e.value.code == DRM_ERR_ARG


def test_create_limits_and_null_arguments():
    import ctypes as C
    from deepreadmapper_amd import ContigTable
    from deepreadmapper_amd._native import DRM_ERR_ARG, lib, ptr
    t = ContigTable([0], [2**40])  # the largest end
    assert t.find(2**40 - REF_LEN, REF_LEN) == 0 and t.find(2**40 - REF_LEN + 1, REF_LEN) == -1
    t.free()
    n = 2**20
    t = ContigTable(np.arange(n, dtype=np.int64) * 3, np.full(n, 2, np.int64))  # the largest table
    assert t.find(3 * (n - 1), 2) == n - 1 and t.find(3 * (n - 1) + 1, 2) == -1 and t.find(3 * 777 + 1, 1) == 777
    t.free()
    a = np.arange(n + 1, dtype=np.int64) * 3
    h = C.c_void_p()
    one = np.ones(n + 1, dtype=np.int64)
    assert lib().drm_contigs_create(ptr(a), ptr(one), n + 1, 0, C.byref(h)) == DRM_ERR_ARG
    assert lib().drm_contigs_create(None, ptr(one), 1, 0, C.byref(h)) == DRM_ERR_ARG
    assert lib().drm_contigs_create(ptr(a), None, 1, 0, C.byref(h)) == DRM_ERR_ARG
    assert lib().drm_contigs_create(ptr(a), ptr(one), 1, 0, None) == DRM_ERR_ARG
    assert lib().drm_contigs_create(ptr(a), ptr(one), 1, -1, C.byref(h)) == DRM_ERR_ARG
    assert lib().drm_contigs_find(None, 0, 0, C.byref(C.c_int32())) == DRM_ERR_ARG
    assert lib().drm_contigs_free(None) == 0
    assert 1 <= lib().drm_contig_lds_max() <= 2**20
