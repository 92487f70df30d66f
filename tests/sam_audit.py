"""An independent auditor of SAM text: every line of a file the pipeline wrote, read as a downstream tool reads it --
from the text, the FASTA and the FASTQ alone. Plain Python and numpy; it imports nothing of the package, of oracle/ or of
the tests' restatements. Its sources are SAMv1 and the definitions of include/drm_hip.h: the scoring of drm_sw_align
(match 1, mismatch 1, a gap base 1: scoring (1, 1, 0, 1)) and of drm_sw_align_affine (a gap of n bases costs open +
n * extend), the clipping penalty of drm_sw_align_affine_clip, the pair fields of drm_sam_pair_fields, the unclipped 5'
end of drm_sam_end5 and the first-seen duplicate rule of drm_dupset, samtools calmd's MD rule.

    findings = audit(lines, contigs, templates, options, truth=None)

lines      the file's lines without their newlines
contigs    {name: bytes} in file order (read_fasta); in reference-header mode {"ref": the whole genome string}
templates  [(name, [(bases, quality)] per mate)] in input order (read_fastq / templates_of); one mate per single read
options    Options: what the run was asked to print
truth      optional {(template index, mate index): Truth}: what a simulator knows about the read

A finding is (line number from 1 or 0 for the file, read name, rule id, message); no finding means the file passed.

What the optimality rules stand on. `align.optimal` is a Gotoh local DP of the read against exactly the printed
reference span: the printed walk lies in the span, so the span's best score is at least AS, and the span lies in the
region the kernel searched, so the kernel's optimum is at least the span's best: without a clipping penalty AS must equal
it; with penalty L, AS - L * (clipped ends) >= best - 2 * L. That span shrinks with every clipped base, so the rule
cannot see an alignment that clips bases it should have aligned. `align.clipped` therefore runs the end-aware DP of
drm_sw_align_affine_clip (plain local at L = 0) over the span widened by the clipped bases, at most Options.flank of them
on either side and never past the contig, and asks AS - L * (clipped ends) to equal its best value. It assumes that those
bases lay in the kernel's region, which holds when the alignment starts no further left of its window than the flank
leaves room for; with flank 0 the span is not widened and the rule says what `align.optimal` says.

The auditor does not check the search's recall (only through a Truth record), nor the MAPQ formula beyond 0..60 and
the anchor values a Truth record names."""
import re
from collections import namedtuple
from dataclasses import dataclass

import numpy as np

Finding = namedtuple("Finding", "line name rule message")
# kind: "map" (must be mapped, on `contig` and strand `reverse`), "unmapped" (must be flag 4: all N), "chance" (random
# bases: flag 4, or as a mate of a pair placed with MAPQ 0, see check_truth), "lenient" (mapped at the truth or
# unmapped). start1: the true 1-based unclipped start (substitution-only reads) or None. sim: (matching columns,
# mismatching columns, gap lengths) of the simulated alignment, whose score AS must reach, or None. places: the
# (contig, start1) of every copy of a repeat the read was drawn from, or None. mapq: the expected value, or None.
Truth = namedtuple("Truth", "kind contig reverse start1 sim places mapq", defaults=(None, False, None, None, None, None))

RULES = (
    "header.hd", "header.sq", "file.columns", "file.primary", "file.order", "file.secondary", "flag.pair_bits",
    "flag.unmapped_bits", "unmapped.fields", "line.rname", "line.bounds", "cigar.grammar", "cigar.qlen", "line.seq",
    "line.qual", "line.mapq", "tag.set", "tag.nm", "tag.md", "tag.as", "align.optimal", "align.clipped", "xa.parse",
    "xa.rname", "xa.bounds", "xa.grammar", "xa.qlen", "xa.nm", "pair.mate_bits", "pair.mate_flags", "pair.next",
    "pair.tlen", "pair.proper", "dup.lines", "dup.mark", "dup.contig_end", "truth.mapped", "truth.place", "truth.start",
    "truth.as", "truth.mapq", "truth.unmapped")


@dataclass
class Options:
    scoring: tuple = (1, 1, 0, 1)  # match, mismatch, open, extend (penalties positive); drm_sw_align is (1, 1, 0, 1)
    clip: int = 0                  # DRM_SAM_CLIP
    flank: int = 0                 # DRM_SAM_FLANK: how far align.clipped widens the span under a clip
    md: bool = False               # MD:Z expected on every mapped line
    qual: bool = False             # column 11 is the FASTQ's quality line, else "*"
    mapq: bool = False             # a real MAPQ; without it every mapped line says 60
    xa: bool = False               # XA:Z allowed on a primary line
    paired: bool = False           # two lines per template with the pair fields
    dup: bool = False              # 1024 on the templates an earlier one shadows; without it 1024 nowhere
    tlen: tuple = None             # (min, max): a proper pair's template length lies inside
    reference_header: bool = False  # the reference's fixed "@SQ SN:ref LN:<header_ln>", RNAME "ref"
    header_ln: int = 150
    per_row: bool = False          # a line per rerank row (no DRM_SAM_LOCI): a row without an alignment is printed with
    #                                its row's bits 16 / 256 beside 4, SEQ oriented by bit 16 as SAMv1 reads that bit


_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def read_fasta(path):
    """{name: sequence bytes} in file order; the name is the first word after '>', letters are upper-cased."""
    out, name = {}, None
    with open(path, "rb") as f:
        for raw in f:
            line = raw.strip()
            if line.startswith(b">"):
                words = line[1:].split()
                name = words[0].decode() if words else ""
                assert name not in out, name
                out[name] = bytearray()
            elif line:
                assert name is not None, "sequence before the first header"
                out[name] += line.upper()
    return {k: bytes(v) for k, v in out.items()}


def read_fastq(path):
    """[(name, bases, quality)]: the name is the header's first word without '@', cut at a '/'."""
    with open(path, "rb") as f:
        rows = f.read().split(b"\n")
    if rows and rows[-1] == b"":
        rows.pop()
    assert len(rows) % 4 == 0, path
    out = []
    for i in range(0, len(rows), 4):
        assert rows[i].startswith(b"@") and rows[i + 2].startswith(b"+"), (path, i)
        name = re.split(rb"[ \t/]", rows[i][1:], maxsplit=1)[0].decode()
        out.append((name, rows[i + 1], rows[i + 3]))
    return out


def templates_of(mate1, mate2=None):
    """The templates of one FASTQ (single reads) or of two (pairs), from read_fastq's lists."""
    if mate2 is None:
        return [(n, [(s, q)]) for n, s, q in mate1]
    assert [n for n, _, _ in mate1] == [n for n, _, _ in mate2]
    return [(n, [(s, q), (s2, q2)]) for (n, s, q), (_, s2, q2) in zip(mate1, mate2)]


# ------------------------------------------------------------------------------------------------ CIGAR and the walk
def parse_cigar(text):
    """[(length, op)] or None when the text is no sequence of <number><letter>."""
    if not re.fullmatch(r"(\d+[A-Za-z=])+", text):
        return None
    return [(int(n), op) for n, op in re.findall(r"(\d+)([A-Za-z=])", text)]


def grammar_errors(runs):
    """What is wrong with a CIGAR as this project prints one; [] when nothing is."""
    bad = []
    ops = [op for _, op in runs]
    if any(op not in "MIDS" for op in ops):
        bad.append("an operation outside MIDS")
    if any(n < 1 for n, _ in runs):
        bad.append("a run of length 0")
    if any(op == "S" and 0 < x < len(ops) - 1 for x, op in enumerate(ops)):
        bad.append("S inside the alignment")
    if any(a == b for a, b in zip(ops, ops[1:])):
        bad.append("two neighbouring runs of one operation")
    core = [op for op in ops if op != "S"]
    if not core or "M" not in core:
        bad.append("no aligned column")
    elif core[0] in "ID" or core[-1] in "ID":
        bad.append("I or D first, last or beside a clip")
    return bad


def query_len(runs):
    return sum(n for n, op in runs if op in "MIS")


def ref_span(runs):
    return sum(n for n, op in runs if op in "MD")


def clips(runs):
    lead = runs[0][0] if runs[0][1] == "S" else 0
    trail = runs[-1][0] if len(runs) > 1 and runs[-1][1] == "S" else 0
    return lead, trail


def walk(contig, pos1, runs, seq, scoring):
    """(NM, MD, score) of the CIGAR walked over the contig from pos1 and over seq; the caller has checked the bounds."""
    ma, mi, go, ge = scoring
    r, q = pos1 - 1, 0
    nm = score = run = 0
    md = []
    for n, op in runs:
        if op == "S":
            q += n
        elif op == "M":
            for x in range(n):
                if contig[r + x] == seq[q + x]:
                    run += 1
                    score += ma
                else:
                    md.append(str(run) + chr(contig[r + x]))
                    run = 0
                    nm += 1
                    score -= mi
            r += n
            q += n
        elif op == "I":
            nm += n
            score -= go + n * ge
            q += n
        elif op == "D":
            md.append(str(run) + "^" + contig[r:r + n].decode())
            run = 0
            nm += n
            score -= go + n * ge
            r += n
    md.append(str(run))
    return nm, "".join(md), score


_NEG = -(1 << 40)


def best_score(ref, read, scoring, clip=0):
    """The largest adj of drm_sw_align_affine_clip (include/drm_hip.h) of `read` (no tags: a = 0, b = len) against
    `ref`, rows over ref and columns over the read; at clip 0 the best score of the plain Gotoh local DP. Integers only.
    E of a row is a running maximum: E[j] = max over k < j of H[k] - open - (j - k) * extend, and since open >= 0 a gap
    opened from a cell that itself ends a gap never beats extending that gap, so H without E serves for H[k]."""
    ma, mi, go, ge = scoring
    m = len(read)
    if m == 0 or len(ref) == 0:
        return 0
    rd = np.frombuffer(read, dtype=np.uint8)
    idx = np.arange(m + 1, dtype=np.int64)
    floor = np.full(m + 1, -clip, dtype=np.int64)
    floor[0] = 0
    end = np.full(m + 1, clip, dtype=np.int64)
    end[m] = 0
    h = floor.copy()
    f = np.full(m + 1, _NEG, dtype=np.int64)
    best = _NEG
    for c in ref:
        s = np.where(rd == c, ma, -mi).astype(np.int64)
        f = np.maximum(h - go - ge, f - ge)
        t = np.empty(m + 1, dtype=np.int64)
        t[0] = 0
        t[1:] = np.maximum(np.maximum(floor[1:], h[:-1] + s), f[1:])
        run = np.maximum.accumulate(t + idx * ge)
        e = np.full(m + 1, _NEG, dtype=np.int64)
        e[1:] = run[:-1] - go - idx[1:] * ge
        h = np.maximum(t, e)
        best = max(best, int((h[1:] - end[1:]).max()))
    return best


# ------------------------------------------------------------------------------------------------ the lines
class _Line:
    def __init__(self, number, text):
        self.number, self.text = number, text
        f = text.split("\t")
        self.ok = len(f) >= 11 and all(re.fullmatch(r"-?\d+", f[x]) for x in (1, 3, 4, 7, 8))
        if not self.ok:
            self.name = f[0]
            return
        self.name, self.flag, self.rname, self.pos, self.mapq, self.cigar = f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5]
        self.rnext, self.pnext, self.tlen, self.seq, self.qual = f[6], int(f[7]), int(f[8]), f[9].encode(), f[10].encode()
        self.tags = f[11:]
        self.unmapped, self.reverse, self.secondary = bool(self.flag & 4), bool(self.flag & 16), bool(self.flag & 256)
        self.runs = None  # the parsed CIGAR of a line that passed the bounds and grammar rules
        self.score = None


class _Audit:
    def __init__(self, lines, contigs, templates, opt, truth):
        self.contigs, self.templates, self.opt, self.truth = contigs, templates, opt, truth or {}
        self.findings = []
        self.lines = lines

    def add(self, line, rule, message):
        assert rule in RULES, rule
        number, name = (line.number, line.name) if isinstance(line, _Line) else (0, "")
        self.findings.append(Finding(number, name, rule, message))

    # -------------------------------------------------------------------------------------------- header
    def header(self):
        head = [x for x in self.lines if x.startswith("@")]
        n = len(head)
        if self.lines[:n] != head:
            self.findings.append(Finding(0, "", "header.hd", "a header line behind the first read"))
        if not head or head[0] != "@HD\tVN:1.0\tSO:unsorted":
            self.findings.append(Finding(1, "", "header.hd", "the first line is not @HD VN:1.0 SO:unsorted"))
        sq = head[1:]
        if self.opt.reference_header:
            want = [f"@SQ\tSN:ref\tLN:{self.opt.header_ln}"]
        else:
            want = [f"@SQ\tSN:{name}\tLN:{len(seq)}" for name, seq in self.contigs.items()]
        if sq != want:
            self.findings.append(Finding(2, "", "header.sq", f"@SQ lines {sq} instead of {want}"))
        return n

    # -------------------------------------------------------------------------------------------- one placement
    def placement(self, line, rname, pos, cigar, seq, rules):
        """The contig, bounds and grammar rules of a printed placement (a line, or an XA entry under other rule ids);
        the parsed CIGAR when all of them passed, else None."""
        if rname not in self.contigs:
            self.add(line, rules["rname"], f"RNAME {rname} is no contig")
            return None
        runs = parse_cigar(cigar)
        bad = ["not a CIGAR"] if runs is None else grammar_errors(runs)
        if bad:
            self.add(line, rules["grammar"], f"CIGAR {cigar}: " + "; ".join(bad))
            return None
        if query_len(runs) != len(seq):
            self.add(line, rules["qlen"], f"CIGAR {cigar} holds {query_len(runs)} query bases, SEQ {len(seq)}")
            return None
        if pos < 1 or pos + ref_span(runs) - 1 > len(self.contigs[rname]):
            self.add(line, rules["bounds"], f"POS {pos} + span {ref_span(runs)} leaves {rname} of {len(self.contigs[rname])}")
            return None
        return runs

    def mapped_line(self, line, bases, quality):
        opt = self.opt
        if line.seq != (revcomp(bases) if line.reverse else bases):
            self.add(line, "line.seq", "SEQ is not the read" + (", reverse-complemented" if line.reverse else ""))
        self.qual(line, quality)
        if opt.mapq:
            if not 0 <= line.mapq <= 60 or (line.secondary and line.mapq != 0):
                self.add(line, "line.mapq", f"MAPQ {line.mapq}" + (" on a secondary line" if line.secondary else ""))
        elif line.mapq != 60:
            self.add(line, "line.mapq", f"MAPQ {line.mapq} without a real MAPQ: the constant is 60")
        keys = [t[:5] for t in line.tags]
        want = ["AS:i:", "NM:i:"] + (["MD:Z:"] if opt.md else [])
        if keys[:len(want)] != want or keys[len(want):] not in ([], ["XA:Z:"]) or \
                (keys[len(want):] and (not opt.xa or line.secondary)):
            self.add(line, "tag.set", f"tags {keys} instead of {want}" + (" [XA:Z:]" if opt.xa else ""))
            return
        tags = {t[:2]: t[5:] for t in line.tags}
        if not re.fullmatch(r"-?\d+", tags["AS"]) or not re.fullmatch(r"\d+", tags["NM"]):
            self.add(line, "tag.set", "AS or NM is no number")
            return
        runs = self.placement(line, line.rname, line.pos, line.cigar, line.seq,
                              dict(rname="line.rname", grammar="cigar.grammar", qlen="cigar.qlen", bounds="line.bounds"))
        if runs is None:
            return
        line.runs, line.score = runs, int(tags["AS"])
        contig = self.contigs[line.rname]
        nm, md, score = walk(contig, line.pos, runs, line.seq, opt.scoring)
        if nm != int(tags["NM"]):
            self.add(line, "tag.nm", f"NM {tags['NM']}, the walk gives {nm}")
        if opt.md and md != tags["MD"]:
            self.add(line, "tag.md", f"MD {tags['MD']}, the walk gives {md}")
        if score != line.score:
            self.add(line, "tag.as", f"AS {line.score}, the walk scores {score}")
        # optimality over the printed span, then over the span widened under the clips
        lo, hi = line.pos - 1, line.pos - 1 + ref_span(runs)
        lead, trail = clips(runs)
        nclip = (lead > 0) + (trail > 0)
        s_span = best_score(contig[lo:hi], line.seq, opt.scoring)
        if (line.score != s_span) if not opt.clip else (line.score - opt.clip * nclip < s_span - 2 * opt.clip):
            self.add(line, "align.optimal", f"AS {line.score} with {nclip} clipped ends, the printed span alone gives {s_span}")
        wide = contig[max(0, lo - min(lead, opt.flank)):min(len(contig), hi + min(trail, opt.flank))]
        s_wide = best_score(wide, line.seq, opt.scoring, opt.clip)
        if line.score - opt.clip * nclip != s_wide:
            self.add(line, "align.clipped", f"AS {line.score} with {nclip} clipped ends is worth {line.score - opt.clip * nclip}"
                                            f", the span with the bases under its clips gives {s_wide}")
        if "XA" in tags:
            self.xa(line, tags["XA"], bases)

    def qual(self, line, quality, oriented=None):
        rev = line.reverse if oriented is None else oriented
        want = b"*" if not self.opt.qual else (quality[::-1] if rev else quality)
        if line.qual != want:
            self.add(line, "line.qual", "QUAL is not the FASTQ's line" + (", reversed" if rev else "") if self.opt.qual
                     else "QUAL is not *")

    def xa(self, line, text, bases):
        entries = re.fullmatch(r"(?:[^,;\t]+,[+-]\d+,[^,;]+,\d+;)+", text)
        if not entries:
            self.add(line, "xa.parse", f"XA:Z:{text} is no list of RNAME,<+|->POS,CIGAR,NM;")
            return
        for rname, sign, pos, cigar, nm in re.findall(r"([^,;\t]+),([+-])(\d+),([^,;]+),(\d+);", text):
            seq = revcomp(bases) if sign == "-" else bases
            runs = self.placement(line, rname, int(pos), cigar, seq,
                                  dict(rname="xa.rname", grammar="xa.grammar", qlen="xa.qlen", bounds="xa.bounds"))
            if runs is None:
                continue
            got = walk(self.contigs[rname], int(pos), runs, seq, self.opt.scoring)[0]
            if got != int(nm):
                self.add(line, "xa.nm", f"XA entry {rname},{sign}{pos},{cigar},{nm}: the walk gives NM {got}")

    def unmapped_line(self, line, bases, quality, mate=None):
        """A flag-4 line: what drm_hip.h (drm_sam_pair_fields) and the README state for it. mate: the other line of a
        pair."""
        opt = self.opt
        bad = []
        oriented = line.reverse and opt.per_row and not opt.paired
        if line.flag & (16 | 256) and not (opt.per_row and not opt.paired):
            self.add(line, "flag.unmapped_bits", f"flag {line.flag}: 4 beside 16 or 256")
        if line.cigar != "*" or line.tlen != 0 or line.tags:
            bad.append("CIGAR, TLEN or tags")
        if line.seq != (revcomp(bases) if oriented else bases):
            bad.append("SEQ is not the read as it came")
        if opt.mapq and line.mapq != 0:
            bad.append(f"MAPQ {line.mapq}")
        if mate is not None and not mate.unmapped:
            if (line.rname, line.pos, line.rnext, line.pnext) != (mate.rname, mate.pos, "=", mate.pos):
                bad.append("RNAME, POS, RNEXT and PNEXT are not the mapped mate's")
        elif opt.per_row and not opt.paired:
            if (line.rname != "*" and line.rname not in self.contigs) or (line.pos, line.rnext, line.pnext) != (0, "*", 0):
                bad.append("RNAME, POS, RNEXT or PNEXT")
        elif (line.rname, line.pos, line.rnext, line.pnext) != ("*", 0, "*", 0):
            bad.append("RNAME, POS, RNEXT or PNEXT")
        if bad:
            self.add(line, "unmapped.fields", "; ".join(bad))
        self.qual(line, quality, oriented)

    # -------------------------------------------------------------------------------------------- pairs
    def pair(self, a, b):
        opt = self.opt
        for m, (x, y) in enumerate(((a, b), (b, a))):
            if x.flag & 0xC1 != (0x41 if m == 0 else 0x81):
                self.add(x, "pair.mate_bits", f"flag {x.flag} on the line of mate {m + 1}")
            if bool(x.flag & 0x8) != y.unmapped or bool(x.flag & 0x20) != (y.reverse and not y.unmapped):
                self.add(x, "pair.mate_flags", f"flag {x.flag} beside the mate's {y.flag}")
        both = not a.unmapped and not b.unmapped
        if both:
            for x, y in ((a, b), (b, a)):
                if (x.rnext, x.pnext) != ("=" if x.rname == y.rname else y.rname, y.pos):
                    self.add(x, "pair.next", f"RNEXT {x.rnext} PNEXT {x.pnext} beside the mate's {y.rname} {y.pos}")
        elif not a.unmapped or not b.unmapped:
            x = b if a.unmapped else a
            if (x.rnext, x.pnext) != ("=", x.pos):
                self.add(x, "pair.next", f"RNEXT {x.rnext} PNEXT {x.pnext} beside an unmapped mate: = and its own POS")
            if x.tlen != 0:
                self.add(x, "pair.tlen", f"TLEN {x.tlen} beside an unmapped mate")
        placed = both and a.runs is not None and b.runs is not None
        if placed:
            if a.rname == b.rname:
                length = max(a.pos + ref_span(a.runs), b.pos + ref_span(b.runs)) - 1 - min(a.pos, b.pos) + 1
                first_is_a = a.pos <= b.pos
                want = (length, -length) if first_is_a else (-length, length)
            else:
                want = (0, 0)
            if (a.tlen, b.tlen) != want:
                self.add(a, "pair.tlen", f"TLEN {a.tlen} and {b.tlen} instead of {want[0]} and {want[1]}")
        for x in (a, b):
            if not x.flag & 0x2:
                continue
            why = None
            if not both:
                why = "a mate is unmapped"
            elif a.rname != b.rname:
                why = "the mates lie on two contigs"
            elif a.reverse == b.reverse:
                why = "the mates lie on one strand"
            elif placed:
                f, r = (b, a) if a.reverse else (a, b)
                f0 = f.pos - clips(f.runs)[0]
                r0, r1 = r.pos - clips(r.runs)[0], r.pos + ref_span(r.runs) - 1 + clips(r.runs)[1]
                if f0 > r0:
                    why = "the reverse mate comes first"
                elif opt.tlen and not opt.tlen[0] <= r1 - f0 + 1 <= opt.tlen[1]:
                    why = f"the template of {r1 - f0 + 1} bases lies outside {opt.tlen}"
            if why:
                self.add(x, "pair.proper", f"flag {x.flag} says proper, but {why}")

    # -------------------------------------------------------------------------------------------- truth
    def check_truth(self, key, line):
        t = self.truth.get(key)
        if t is None:
            return
        opt = self.opt
        if t.kind in ("unmapped", "chance"):
            # drm_pair_hits takes every live row (score > 0) of a mate as a hit, and the paired path has no chance level
            # as DRM_SAM_LOCI's single reads have: a random mate is placed on its best chance alignment, with MAPQ 0
            placed_by_chance = t.kind == "chance" and opt.paired and (line.mapq == 0 or not opt.mapq)
            if not line.unmapped and not placed_by_chance:
                self.add(line, "truth.unmapped", "a read that can map nowhere is mapped" +
                         (f" with MAPQ {line.mapq}" if t.kind == "chance" else ""))
            return
        if line.unmapped:
            if t.kind == "map":
                self.add(line, "truth.mapped", "a read of a must-map class is unmapped")
            return
        places = t.places or [(t.contig, t.start1)]
        if line.rname not in {c for c, _ in places} or line.reverse != t.reverse:
            self.add(line, "truth.place", f"on {line.rname}, strand {'-' if line.reverse else '+'}: the truth is "
                                          f"{places}, strand {'-' if t.reverse else '+'}")
            return
        if line.runs is None:
            return
        start = line.pos - clips(line.runs)[0]
        starts = {s for c, s in places if c == line.rname and s is not None}
        if starts and start not in starts:
            self.add(line, "truth.start", f"unclipped start {start}: the truth is {sorted(starts)}")
        if t.sim is not None:
            ma, mi, go, ge = opt.scoring
            least = ma * t.sim[0] - mi * t.sim[1] - sum(go + ge * n for n in t.sim[2])
            if line.score < least:
                self.add(line, "truth.as", f"AS {line.score}: the simulated alignment scores {least}")
        if opt.mapq and t.mapq is not None and line.mapq != t.mapq:
            self.add(line, "truth.mapq", f"MAPQ {line.mapq}: the truth is {t.mapq}")

    # -------------------------------------------------------------------------------------------- the file
    def run(self):
        opt = self.opt
        nhead = self.header()
        body = [_Line(nhead + 1 + i, x) for i, x in enumerate(self.lines[nhead:]) if not x.startswith("@")]
        for line in body:
            if not line.ok:
                self.add(line, "file.columns", "fewer than eleven columns, or a number column that holds none")
        if any(not x.ok for x in body):
            return self.findings
        records = []
        for line in body:
            if not line.secondary:
                records.append([line])
            elif not records or records[-1][0].name != line.name or records[-1][0].unmapped and not opt.per_row:
                self.add(line, "file.secondary", "a secondary line that follows no primary line of its read")
                return self.findings
            else:
                records[-1].append(line)
        slots = [(t, m) for t, (_, mates) in enumerate(self.templates) for m in range(len(mates))]
        if len(records) != len(slots):
            self.findings.append(Finding(0, "", "file.primary", f"{len(records)} lines without 256 for {len(slots)} reads"))
            return self.findings
        for (t, m), rec in zip(slots, records):
            name, mates = self.templates[t]
            bases, quality = mates[m]
            if rec[0].name != name:
                self.add(rec[0], "file.order", f"the read at this place of the input is {name}")
                continue
            for line in rec:
                paired_bits = line.flag & (0x1 | 0x2 | 0x8 | 0x20 | 0x40 | 0x80)
                if paired_bits and not opt.paired:
                    self.add(line, "flag.pair_bits", f"flag {line.flag} in a run of single reads")
                elif opt.paired and paired_bits and not line.flag & 0x1:
                    self.add(line, "flag.pair_bits", f"flag {line.flag}: pair bits without 1")
                if opt.paired and line.secondary:
                    self.add(line, "file.secondary", "a secondary line in a paired file")
                if not line.unmapped:
                    self.mapped_line(line, bases, quality)
                elif not opt.paired:
                    self.unmapped_line(line, bases, quality)
        if opt.paired:
            for t in range(len(self.templates)):
                a, b = records[2 * t][0], records[2 * t + 1][0]
                if a.name != self.templates[t][0] or b.name != a.name:
                    continue
                for x, y, m in ((a, b, 0), (b, a, 1)):
                    if x.unmapped:
                        self.unmapped_line(x, *self.templates[t][1][m], mate=y)
                self.pair(a, b)
        for (t, m), rec in zip(slots, records):
            if rec[0].name == self.templates[t][0]:
                self.check_truth((t, m), rec[0])
        self.duplicates(records)
        return self.findings

    def duplicates(self, records):
        """1024 on all lines of a template iff an earlier template had its key: the unordered pair of (contig, unclipped
        5' end, strand) of its mapped primaries (drm_hip.h: what samtools derives from the printed line)."""
        per = 2 if self.opt.paired else 1
        seen = set()
        for t in range(len(self.templates)):
            recs = records[per * t:per * t + per]
            lines = [x for rec in recs for x in rec]
            ends = []
            for rec in recs:
                x = rec[0]
                if x.unmapped or x.runs is None:
                    continue
                lead, trail = clips(x.runs)
                end = x.pos + ref_span(x.runs) - 1 + trail if x.reverse else x.pos - lead
                if not 1 <= end <= len(self.contigs[x.rname]):
                    self.add(x, "dup.contig_end", f"the unclipped 5' end {end} lies outside {x.rname}: the contig-local key "
                                                  "is not the header's genome-string key here")
                ends.append((x.rname, end, x.reverse))
            if any(not x.unmapped and x.runs is None for rec in recs for x in rec[:1]):
                continue  # a primary whose placement failed its own rules has no end to key by
            key = tuple(sorted(ends)) if ends else None
            marks = {bool(x.flag & 1024) for x in lines}
            want = self.opt.dup and key is not None and key in seen
            if key is not None:
                seen.add(key)
            if len(marks) > 1:
                self.add(lines[0], "dup.lines", "1024 on some lines of the template only")
            elif marks != {want}:
                self.add(lines[0], "dup.mark", ("1024 without an earlier template of these ends" if not want else
                                                f"no 1024 although an earlier template had the ends {key}"))


def audit(lines, contigs, templates, options, truth=None):
    return _Audit(list(lines), contigs, templates, options, truth).run()


def report(findings):
    return "\n".join(f"line {f.line} {f.name} [{f.rule}] {f.message}" for f in findings)
