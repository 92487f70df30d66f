"""GPU test of bin/pipeline's DRM_SAM_LOCI with DRM_CONTIGS=1 (test_gpu_contigs_cli's fixture: four contigs, chrD
repeating chrC's last window): the loci are found on the spread ids, so the read from that window has two placements,
one on chrC and one on chrD 151 bases on in the genome string, although both lie within DRM_MAPQ_SPAN=200 of each
other; RNAME and POS of a secondary line and of an XA entry are the contig's own; the primary line of a read that stays
mapped is its line of the run without the switch; the XA entries are the secondary lines of the other form."""
import re

import pytest

from test_gpu_contigs_cli import MAPQ_SPAN, _composed_single, _header, _sam, fixture  # noqa: F401

pytestmark = pytest.mark.gpu


def _groups(lines, nhead):
    out = []
    for line in lines[nhead:]:
        if not int(line.split("\t")[1]) & 256:
            out.append([])
        out[-1].append(line)
    return out


def test_loci_on_the_spread_ids_with_contig_names_and_positions(fixture):
    fx = fixture
    more = dict(DRM_CONTIGS="1", DRM_SAM_CIGAR="1", DRM_SAM_MAPQ="1", DRM_MAPQ_SPAN=str(MAPQ_SPAN))
    nhead = len(_header(fx))
    out = {}
    for name, extra in (("lines", dict(DRM_SAM_LOCI="5")), ("xa", dict(DRM_SAM_LOCI="5", DRM_SAM_XA="1")),
                        ("lines_b4", dict(DRM_SAM_LOCI="5", DRM_SAM_BLOCK="4"))):
        r = fx["run"]("ix", fx["tmp"] / "reads.fastq", fx["fa"], "loci_" + name, ["1", "1"], **more, **extra)
        assert r.returncode == 0, r.stdout + r.stderr
        out[name] = _sam(fx["tmp"] / ("loci_" + name) / "results.sam")
    assert out["lines_b4"] == out["lines"] and out["lines"][:nhead] == _header(fx)
    before = _composed_single(fx, mapq=True)  # the file without the switch, as test_gpu_contigs_cli pins it
    old = {g[0].split("\t")[0]: g for g in _groups(before, nhead)}
    new, xa = _groups(out["lines"], nhead), out["xa"][nhead:]
    assert [g[0].split("\t")[0] for g in new] == [f"read{i}" for i in range(len(fx["reads"]))] and len(xa) == len(new)
    mapped = 0
    for group, line in zip(new, xa):
        f = group[0].split("\t")
        assert len(group) <= 5
        if int(f[1]) & 4:
            assert f[1:9] == ["4", "*", "0", "0", "*", "*", "0", "0"] and len(group) == 1 and line == group[0]
            continue
        mapped += 1
        assert group[0] == old[f[0]][0]  # the primary line is the one of before
        # the XA form: the same primary, and one entry per secondary line of the other form, in its order
        assert line.partition("\tXA:Z:")[0] == group[0]
        entries = re.findall(r"([^,;]+),([+-])(\d+),([0-9MIDS]+),(\d+);", line.partition("\tXA:Z:")[2])
        want = [(s[2], "-" if int(s[1]) & 16 else "+", s[3], s[5], s[12][5:]) for s in (x.split("\t") for x in group[1:])]
        assert entries == want and all(int(s.split("\t")[1]) & 256 and s.split("\t")[4] == "0" for s in group[1:])
    assert 0 < mapped < len(new)
    # the seam read: chrC's last window and chrD, 151 bases apart in the genome string, are two loci, with MAPQ 0
    i = fx["truth"].index((2, 250, False))
    places = sorted((x.split("\t")[2], x.split("\t")[3], x.split("\t")[5]) for x in new[i])
    assert places == [("chrC", "251", "150M"), ("chrD", "1", "150M")] and new[i][0].split("\t")[4] == "0"
    assert re.search(r"\tXA:Z:chr[CD],\+(251|1),150M,0;$", xa[i])
    assert len(new[0]) == 1 and new[0][0].split("\t")[4] == "60"  # read0, unique on chrA
