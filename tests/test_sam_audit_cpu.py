"""The SAM auditor (tests/sam_audit.py) catches what it claims, without a GPU and without the pipeline. A small simulator
builds SAM files that are correct by construction -- POS, CIGAR, NM, MD and AS come from the edit script it applied to
the genome, the pair fields and the duplicate marks from the placements it chose, never from the auditor -- over three
contigs with one duplicated stretch and the read classes of tests/test_gpu_sam_audit_cli.py. The auditor finds nothing
in them: single reads with secondary lines, single reads under a clipping penalty with XA, pairs, and the line-per-row
form under the reference's header. Then one field is falsified at a time, and the auditor must name the rule that field
breaks and no rule beyond those that follow from the same falsified field. Its numpy DP is pinned to a naive triple
loop on random read / span pairs, linear gaps (open = 0) and the clipping penalty included."""
import numpy as np
import pytest

import sam_audit as A

READ = 50
AFFINE = (1, 4, 6, 1)
OTHER = dict(zip(b"ACGT", b"CGTA"))


def _genome():
    rng = np.random.default_rng(2024)
    rand = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).astype(np.uint8))  # noqa: E731
    c0 = bytearray(rand(320))
    c0[220:280] = c0[40:100]  # the duplicated stretch
    return {"c0": bytes(c0), "c1": rand(260), "c2": rand(200)}, rng


# ------------------------------------------------------------------------------------------------ the simulator
def _subs(offsets, length=READ):
    """The script of a read of `length` reference bases with substitutions at the forward offsets."""
    out, at = [], 0
    for o in sorted(offsets):
        if o > at:
            out.append(("=", o - at))
        out.append(("X", 1))
        at = o + 1
    if at < length:
        out.append(("=", length - at))
    return out


def _place(contigs, contig, start0, reverse, script, scoring, clip):
    """One placement by construction: the forward-strand read of the script walked over contig from start0, its ends
    clipped where a local alignment under (scoring, clip) clips them, and POS, CIGAR, NM, MD, AS of what remains."""
    ma, mi, go, ge = scoring
    ref = contigs[contig]
    read, at = bytearray(), start0
    for op, n in script:
        if op == "=":
            read += ref[at:at + n]
            at += n
        elif op == "X":
            read.append(OTHER[ref[at]])
            at += 1
        elif op == "D":
            at += n
        else:  # "I": the bases themselves
            read += n
    total_span = at - start0
    assert at <= len(ref)
    script = list(script)
    lead = trail = 0
    # a mismatch k <= 3 bases from an end: aligned when its k matches less the mismatch beat the price of the clip
    if len(script) > 2 and script[0][0] == "=" and script[0][1] <= 3 and script[1][0] == "X":
        k = script[0][1]
        if k * ma - mi <= -clip:
            lead, script = k + 1, script[2:]
    if len(script) > 2 and script[-1][0] == "=" and script[-1][1] <= 3 and script[-2][0] == "X":
        k = script[-1][1]
        if k * ma - mi <= -clip:
            trail, script = k + 1, script[:-2]
    pos0 = start0 + lead
    runs, md, run, nm, score, at = [], "", 0, 0, 0, pos0
    for op, n in script:
        sam = "M" if op in "=X" else op
        length = len(n) if op == "I" else n
        if runs and runs[-1][1] == sam:
            runs[-1][0] += length
        else:
            runs.append([length, sam])
        if op == "=":
            run += n
            score += ma * n
            at += n
        elif op == "X":
            md += str(run) + chr(ref[at])
            run, nm, score, at = 0, nm + 1, score - mi, at + 1
        elif op == "D":
            md += str(run) + "^" + ref[at:at + n].decode()
            run, nm, score, at = 0, nm + n, score - go - ge * n, at + n
        else:
            nm, score = nm + length, score - go - ge * length
    md += str(run)
    cigar = (f"{lead}S" if lead else "") + "".join(f"{n}{op}" for n, op in runs) + (f"{trail}S" if trail else "")
    return dict(mapped=True, contig=contig, pos=pos0 + 1, span=at - pos0, reverse=reverse, cigar=cigar, nm=nm, md=md,
                score=score, fwd=bytes(read), start1=start0 + 1, end5=start0 + total_span if reverse else start0 + 1,
                mapq=60, alts=[])


def _reads(contigs, rng, scoring, clip):
    """{name: placement}: the read classes, each a dict as _place makes it plus the read as the FASTQ holds it."""
    def p(contig, start0, reverse, script=None):
        return _place(contigs, contig, start0, reverse, script or [("=", READ)], scoring, clip)
    out = {
        "exact_f": p("c0", 110, False), "exact_r": p("c1", 70, True),
        "first_base": p("c1", 0, False), "last_base": p("c2", len(contigs["c2"]) - READ, True),
        "sub2_f": p("c0", 150, False, _subs([1])), "sub2_r": p("c1", 120, True, _subs([READ - 2])),
        "sub49_f": p("c2", 30, False, _subs([READ - 2])), "sub49_r": p("c2", 90, True, _subs([1])),
        "two_subs": p("c1", 180, False, _subs([20, 31])),
        "del3": p("c0", 130, False, [("=", 22), ("D", 3), ("=", 28)]),
        "ins2": p("c1", 30, True, [("=", 27), ("I", b"GT"), ("=", 21)]),
        "clip_ins": p("c2", 60, False, [("=", 1), ("X", 1), ("=", 20), ("I", b"C"), ("=", 27)]),
        "rep_a": p("c0", 45, False), "rep_b": p("c0", 225, True),
    }
    for name, other in (("rep_a", 225), ("rep_b", 45)):
        r = out[name]
        r["mapq"] = 0
        r["alts"] = [dict(r, pos=other + 1, alts=[])]
    for r in out.values():
        r["bases"] = A.revcomp(r["fwd"]) if r["reverse"] else r["fwd"]
    out["all_n"] = dict(mapped=False, bases=b"N" * READ)
    out["random"] = dict(mapped=False, chance=True, bases=bytes(rng.choice(list(b"ACGT"), size=READ).astype(np.uint8)))
    # a mate that can map nowhere, placed by the pairing on a chance alignment of 20 bases (drm_pair_hits has no chance
    # level): MAPQ 0. The N behind them match nothing, so the 20 columns are the best local alignment by construction.
    ch = p("c1", 100, False, [("=", 20)])
    ch.update(fwd=ch["fwd"] + b"N" * (READ - 20), cigar="20M30S", mapq=0, chance=True)
    ch["bases"], out["chance"] = ch["fwd"], ch
    # the repeats of the duplicate rule: exact_f again, and sub2_f's fragment without its substitution (another POS
    # where the end is clipped, the same unclipped 5' end)
    out["dup_exact"] = dict(out["exact_f"])
    out["dup_end"] = p("c0", 150, False)
    out["dup_end"]["bases"] = out["dup_end"]["fwd"]
    # mates for the pair shapes
    for name, r in (("m_r300", p("c0", 260, True)), ("m_r_same", p("c0", 110, True)), ("m_f_far", p("c0", 10, False)),
                    ("m_c1_r", p("c1", 200, True)), ("m_del_r", p("c0", 200, True, [("=", 30), ("D", 3), ("=", 20)]))):
        r["bases"] = A.revcomp(r["fwd"]) if r["reverse"] else r["fwd"]
        out[name] = r
    for r in out.values():
        q = bytes(rng.integers(35, 74, size=READ).astype(np.uint8))
        r["quality"] = q if q != q[::-1] else b"#" + q[1:-1] + b"I"
    out["dup_exact"]["quality"] = out["exact_f"]["quality"][::-1]
    return out


def _line(name, flag, r, opt, names, secondary=False, mate=None, tlen=0, xa=True):
    """One SAM line of placement r; names maps a contig to (RNAME, offset)."""
    rev = r.get("reverse", False) and r["mapped"]
    qual = (r["quality"][::-1] if rev else r["quality"]).decode() if opt.qual else "*"
    rnext, pnext = "*", 0
    if mate is not None and (r["mapped"] or mate["mapped"]):
        near, far = (r if r["mapped"] else mate), (mate if mate["mapped"] else r)
        rnext = "=" if names[near["contig"]][0] == names[far["contig"]][0] else names[far["contig"]][0]
        pnext = far["pos"] + names[far["contig"]][1]
    if not r["mapped"]:
        rname, pos = "*", 0
        if mate is not None and mate["mapped"]:
            rname, pos = names[mate["contig"]][0], mate["pos"] + names[mate["contig"]][1]
        return [name, str(flag | 4), rname, str(pos), "0" if opt.mapq else "60", "*", rnext, str(pnext), "0",
                r["bases"].decode(), qual]
    rname, off = names[r["contig"]]
    mapq = (0 if secondary else r["mapq"]) if opt.mapq else 60
    f = [name, str(flag | (16 if rev else 0) | (256 if secondary else 0)), rname, str(r["pos"] + off), str(mapq),
         r["cigar"], rnext, str(pnext), str(tlen), r["fwd"].decode(), qual, f"AS:i:{r['score']}", f"NM:i:{r['nm']}"]
    if opt.md:
        f.append("MD:Z:" + r["md"])
    if opt.xa and xa and r["alts"] and not secondary:
        f.append("XA:Z:" + "".join(f"{names[a['contig']][0]},{'-' if a['reverse'] else '+'}{a['pos'] + names[a['contig']][1]},"
                                   f"{a['cigar']},{a['nm']};" for a in r["alts"]))
    return f


SINGLE = ["exact_f", "exact_r", "first_base", "last_base", "sub2_f", "sub2_r", "sub49_f", "sub49_r", "two_subs", "del3",
          "ins2", "clip_ins", "rep_a", "rep_b", "all_n", "random", "dup_exact", "dup_end", "all_n", "rep_a"]
PAIRS = [("fr", "exact_f", "m_r300"), ("fr_edits", "sub2_f", "m_del_r"), ("tie", "exact_f", "m_r_same"),
         ("same_strand", "m_f_far", "exact_f"), ("rf", "m_r_same", "dup_end"), ("two_contigs", "exact_f", "m_c1_r"),
         ("one_n", "two_subs", "all_n"), ("n_one", "all_n", "exact_r"), ("both_n", "all_n", "all_n"),
         ("fr_again", "exact_f", "m_r300"), ("fr_swapped", "m_r300", "exact_f"), ("rep_pair", "rep_a", "m_r300"),
         ("both_n_again", "all_n", "all_n"), ("one_n_again", "two_subs", "all_n"), ("chance_mate", "chance", "random")]
WINDOW = (READ, 260)


def _truth(r):
    if r.get("chance"):
        return A.Truth("chance")
    if not r["mapped"]:
        return A.Truth("unmapped")
    places = [(r["contig"], r["start1"])] + [(a["contig"], a["start1"] + a["pos"] - r["pos"]) for a in r["alts"]]
    return A.Truth("map", r["contig"], r["reverse"], r["start1"] if "D" not in r["cigar"] and "I" not in r["cigar"] else None,
                   None, places if r["alts"] else None, r["mapq"])


def build(form, scoring=AFFINE, clip=0, flank=16):
    """(lines as field lists, contigs, templates, options, truth) of one constructed file. form: "single" (secondary
    lines), "single_xa", "paired" (XA), "per_row" (the reference's header, RNAME ref over the one genome string, a line
    per row: every read gets its placement twice more as rows without an alignment on either strand)."""
    contigs, rng = _genome()
    reads = _reads(contigs, rng, scoring, clip)
    per_row = form == "per_row"
    opt = A.Options(scoring=scoring, clip=clip, flank=flank, md=not per_row, qual=not per_row, mapq=not per_row,
                    xa=form in ("single_xa", "paired"), paired=form == "paired", dup=not per_row,
                    tlen=WINDOW if form == "paired" else None, reference_header=per_row, per_row=per_row)
    names = {c: (c, 0) for c in contigs}
    header = ["@HD\tVN:1.0\tSO:unsorted"] + [f"@SQ\tSN:{c}\tLN:{len(s)}" for c, s in contigs.items()]
    if per_row:
        off = np.cumsum([0] + [len(s) for s in contigs.values()])
        names = {c: ("ref", int(o)) for c, o in zip(contigs, off)}
        header = header[:1] + ["@SQ\tSN:ref\tLN:150"]
        contigs = {"ref": b"".join(contigs.values())}
    lines, templates, truth, seen = [], [], {}, set()
    if form != "paired":
        for t, key in enumerate(SINGLE):
            r = reads[key]
            name = f"s{t}_{key}"
            k = (r["contig"], r["end5"], r["reverse"]) if r["mapped"] else None
            dup = 1024 if opt.dup and k is not None and k in seen else 0
            seen.add(k)  # None, the template without a mapped mate, is never looked up
            lines.append(_line(name, dup, r, opt, names))
            if r["mapped"] and not opt.xa:
                lines += [_line(name, dup, dict(a, quality=r["quality"]), opt, names, secondary=True) for a in r["alts"]]
            if per_row:  # rows without an alignment: 4 beside the row's own bits, SEQ oriented by bit 16
                lines.append([name, "260", "ref", "0", "60", "*", "*", "0", "0", r["bases"].decode(), "*"])
                lines.append([name, "276", "ref", "0", "60", "*", "*", "0", "0", A.revcomp(r["bases"]).decode(), "*"])
            templates.append((name, [(r["bases"], r["quality"])]))
            if not per_row:
                truth[(t, 0)] = _truth(r)
    else:
        for t, (name, k1, k2) in enumerate(PAIRS):
            a, b = reads[k1], reads[k2]
            keys = sorted((r["contig"], r["end5"], r["reverse"]) for r in (a, b) if r["mapped"])
            k = tuple(keys) if keys else None
            dup = 1024 if k is not None and k in seen else 0
            seen.add(k)  # None, the template without a mapped mate, is never looked up
            both = a["mapped"] and b["mapped"]
            proper, tl = False, (0, 0)
            if both and a["contig"] == b["contig"]:
                length = max(a["pos"] + a["span"], b["pos"] + b["span"]) - 1 - min(a["pos"], b["pos"]) + 1
                tl = (length, -length) if a["pos"] <= b["pos"] else (-length, length)
                f, r = (b, a) if a["reverse"] else (a, b)
                proper = a["reverse"] != b["reverse"] and f["start1"] <= r["start1"] and \
                    WINDOW[0] <= r["start1"] + READ - f["start1"] <= WINDOW[1]
            for m, (x, y) in enumerate(((a, b), (b, a))):
                flag = 1 | (0x40, 0x80)[m] | (0 if y["mapped"] else 8) | (32 if y["mapped"] and y["reverse"] else 0) | \
                    (2 if proper else 0) | dup
                lines.append(_line(name, flag, x, opt, names, mate=y, tlen=tl[m]))
                truth[(t, m)] = _truth(x)
            templates.append((name, [(a["bases"], a["quality"]), (b["bases"], b["quality"])]))
    return header, lines, contigs, templates, opt, truth


def _audit(built, lines=None):
    header, own, contigs, templates, opt, truth = built
    return A.audit(header + ["\t".join(f) for f in (own if lines is None else lines)], contigs, templates, opt, truth)


FORMS = {"single": dict(form="single"), "single_clip": dict(form="single_xa", clip=5), "paired": dict(form="paired", clip=5),
         "paired_local": dict(form="paired"), "per_row": dict(form="per_row", scoring=(1, 1, 0, 1), flank=0),
         "single_legacy": dict(form="single", scoring=(1, 1, 0, 1), flank=0)}


@pytest.fixture(scope="module")
def built():
    return {k: build(**v) for k, v in FORMS.items()}


@pytest.mark.parametrize("form", list(FORMS))
def test_the_constructed_files_have_no_finding(built, form):
    found = _audit(built[form])
    assert not found, A.report(found)
    _, lines, _, templates, opt, _ = built[form]
    flags = [int(f[1]) for f in lines]
    # the file holds what the mutations below stand on
    assert any(x & 16 for x in flags) and any(x & 4 for x in flags) and (not opt.dup or sum(bool(x & 1024) for x in flags) >= 3)
    assert any("D" in f[5] for f in lines)
    if form == "single":
        assert any("S" in f[5] for f in lines) and any("I" in f[5] for f in lines)
        assert any(x & 256 for x in flags) and [f[5] for f in lines if f[0].endswith("sub2_f")] == ["2S48M"]
    if form == "single_clip":
        assert any(t.startswith("XA:Z:") for f in lines for t in f[11:])
        assert [(f[5], f[12]) for f in lines if "sub2" in f[0] or "sub49" in f[0]] == [("50M", "NM:i:1")] * 4
    if form == "paired":
        assert {x & 2 for x in flags} == {0, 2} and len(templates) == len(lines) // 2
    if form == "per_row":
        assert any(x & 4 and x & 16 and x & 256 for x in flags)


def _find(lines, name, nth=0):
    return [i for i, f in enumerate(lines) if f[0].split("_", 1)[-1] == name or f[0] == name][nth]


def _set(f, **kw):
    cols = dict(flag=1, rname=2, pos=3, mapq=4, cigar=5, rnext=6, pnext=7, tlen=8, seq=9, qual=10)
    f = list(f)
    for k, v in kw.items():
        if k in cols:
            f[cols[k]] = str(v)
        else:  # a tag
            x = [i for i, t in enumerate(f) if t.startswith(k + ":")][0]
            f[x] = f[x][:5] + str(v)
    return f


def _tag(f, key):
    return [t[5:] for t in f if t.startswith(key + ":")][0]


WALK = {"tag.nm", "tag.md", "tag.as"}
SCORE = {"align.optimal", "align.clipped"}


def _mutations():
    """(id, form, mutate(lines) in place, rules that must be named, further rules that follow from the same field)."""
    def on(name, nth, fn):
        def go(lines):
            i = _find(lines, name, nth)
            lines[i] = fn(lines[i])
        return go

    def pos_plus_1(f):
        return _set(f, pos=int(f[3]) + 1)

    def swap_runs(f):
        runs = A.parse_cigar(f[5])
        assert len(runs) == 3 and runs[0][0] != runs[2][0]
        return _set(f, cigar="".join(f"{n}{op}" for n, op in (runs[2], runs[1], runs[0])))

    def ins_to_clip(f):
        assert f[5] == "2S20M1I27M"
        return _set(f, cigar="2S1I47M")

    def md_base(f):
        md = _tag(f, "MD:Z")
        x = [i for i, c in enumerate(md) if c.isalpha()][0]
        return _set(f, **{"MD:Z": md[:x] + chr(OTHER[ord(md[x])]) + md[x + 1:]})

    def md_count(f):
        md = _tag(f, "MD:Z")
        x = [i for i, c in enumerate(md) if c.isalpha()][0]
        return _set(f, **{"MD:Z": str(int(md[:x]) + 1) + md[x:]})

    def clip_ten_good_bases(f):
        assert f[5] == "50M" and not int(f[1]) & 16
        return _set(f, pos=int(f[3]) + 10, cigar="10S40M", **{"AS:i": 40, "MD:Z": "40"})

    def clip_the_mismatch(f):  # under the penalty 5: 50M with its mismatch is worth 45, the clipped line 48 - 5
        assert f[5] == "50M" and _tag(f, "NM:i") == "1" and _tag(f, "AS:i") == "45" and _tag(f, "MD:Z")[:1] == "1"
        return _set(f, pos=int(f[3]) + 2, cigar="2S48M", **{"AS:i": 48, "NM:i": 0, "MD:Z": "48"})

    def unreversed(col):
        def go(f):
            assert int(f[1]) & 16
            return _set(f, **{col: A.revcomp(f[9].encode()).decode() if col == "seq" else f[10][::-1]})
        return go

    def xa_sign(f):
        xa = _tag(f, "XA:Z")
        return _set(f, **{"XA:Z": xa.replace(",-", ",+", 1) if ",-" in xa else xa.replace(",+", ",-", 1)})

    def pair(name, fn):
        def go(lines):
            i = _find(lines, name)
            lines[i], lines[i + 1] = fn(lines[i], lines[i + 1])
        return go

    def move_1024(lines):
        first, second = _find(lines, "exact_f"), _find(lines, "dup_exact")
        assert int(lines[second][1]) & 1024 and not int(lines[first][1]) & 1024
        lines[first] = _set(lines[first], flag=int(lines[first][1]) | 1024)
        lines[second] = _set(lines[second], flag=int(lines[second][1]) & ~1024)

    def starts_only(a, b):
        n = abs(int(b[3]) - int(a[3])) + 1
        return _set(a, tlen=n), _set(b, tlen=-n)

    return [
        ("pos+1 forward", "single", on("exact_f", 0, pos_plus_1), WALK, SCORE | {"truth.start", "dup.mark"}),
        ("pos+1 reverse", "single", on("exact_r", 0, pos_plus_1), WALK, SCORE | {"truth.start", "dup.mark"}),
        ("cigar runs swapped", "single", on("del3", 0, swap_runs), WALK, SCORE | {"truth.as"}),
        ("1I beside the clip", "single", on("clip_ins", 0, ins_to_clip), {"cigar.grammar"}, set()),
        ("nm-1", "single", on("two_subs", 0, lambda f: _set(f, **{"NM:i": int(_tag(f, "NM:i")) - 1})), {"tag.nm"}, set()),
        ("md base", "single", on("two_subs", 0, md_base), {"tag.md"}, set()),
        ("md count", "single", on("two_subs", 0, md_count), {"tag.md"}, set()),
        ("as+1", "single", on("two_subs", 0, lambda f: _set(f, **{"AS:i": int(_tag(f, "AS:i")) + 1})), {"tag.as"}, SCORE),
        ("suboptimal: ten good bases clipped", "single", on("exact_f", 0, clip_ten_good_bases), {"align.clipped"}, set()),
        ("seq not reverse-complemented", "single", on("exact_r", 0, unreversed("seq")), {"line.seq"}, WALK | SCORE),
        ("qual not reversed", "single", on("exact_r", 0, unreversed("qual")), {"line.qual"}, set()),
        ("secondary with mapq 5", "single", on("rep_a", 1, lambda f: _set(f, mapq=5)), {"line.mapq"}, set()),
        ("xa sign flipped", "single_clip", on("rep_a", 0, xa_sign), {"xa.nm"}, set()),
        ("0x20 cleared", "paired", on("fr", 0, lambda f: _set(f, flag=int(f[1]) & ~0x20)), {"pair.mate_flags"}, set()),
        ("pnext off by one", "paired", on("fr", 0, lambda f: _set(f, pnext=int(f[7]) + 1)), {"pair.next"}, set()),
        ("tlen signs swapped", "paired", pair("fr", lambda a, b: (_set(a, tlen=b[8]), _set(b, tlen=a[8]))), {"pair.tlen"}, set()),
        ("tlen from the starts only", "paired", pair("fr", starts_only), {"pair.tlen"}, set()),
        ("0x2 on a same-strand pair", "paired",
         pair("same_strand", lambda a, b: (_set(a, flag=int(a[1]) | 2), _set(b, flag=int(b[1]) | 2))), {"pair.proper"}, set()),
        ("1024 on the first occurrence", "single", move_1024, {"dup.mark"}, set()),
        ("1024 on one line of two", "paired", on("fr_again", 0, lambda f: _set(f, flag=int(f[1]) & ~1024)), {"dup.lines"}, set()),
        ("one base past the contig", "single", on("last_base", 0, pos_plus_1), {"line.bounds"}, set()),
        ("a chance placement with mapq 7", "paired", on("chance_mate", 0, lambda f: _set(f, mapq=7)), {"truth.unmapped"}, set()),
        ("a mismatch clipped under the penalty", "single_clip", on("sub2_f", 0, clip_the_mismatch), {"align.clipped"}, set()),
    ]


MUTATIONS = _mutations()


@pytest.mark.parametrize("case", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_one_falsified_field_is_named_by_its_rule(built, case):
    _, form, mutate, must, may = case
    lines = [list(f) for f in built[form][1]]
    mutate(lines)
    assert lines != built[form][1]
    found = _audit(built[form], lines)
    rules = {f.rule for f in found}
    assert must <= rules and rules <= must | may, A.report(found)
    assert rules <= set(A.RULES)


# ------------------------------------------------------------------------------------------------ the DP
def naive_best(ref, read, scoring, clip):
    """drm_sw_align_affine_clip's recurrence as include/drm_hip.h writes it, cell by cell, E and F as explicit maxima
    over every gap length; the largest adj, tags absent (a = 0, b = len(read))."""
    ma, mi, go, ge = scoring
    n, m = len(ref), len(read)
    neg = -10 ** 9
    floor = lambda j: 0 if j <= 0 else -clip  # noqa: E731
    H = [[0] * (m + 1) for _ in range(n + 1)]
    for j in range(m + 1):
        H[0][j] = floor(j)
    best = neg
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            s = ma if ref[i - 1] == read[j - 1] else -mi
            f = max([H[i - g][j] - go - ge * g for g in range(1, i + 1)])
            e = max([H[i][j - g] - go - ge * g for g in range(1, j + 1)])
            H[i][j] = max(floor(j), H[i - 1][j - 1] + s, f, e)
            best = max(best, H[i][j] - (0 if j == m else clip))
    return best


def test_the_numpy_dp_is_the_naive_triple_loop():
    rng = np.random.default_rng(7)
    for trial in range(60):
        scoring = [(1, 1, 0, 1), (1, 4, 6, 1), (2, 3, 0, 2), (1, 2, 3, 2), (3, 5, 4, 1)][trial % 5]
        clip = (0, 0, 5, 2, 9, 0)[trial % 6]
        n, m = int(rng.integers(1, 26)), int(rng.integers(1, 22))
        alphabet = list(b"ACGT") if trial % 4 else list(b"AC")  # two letters: many gaps and ties
        ref = bytes(rng.choice(alphabet, size=n).astype(np.uint8))
        if trial % 3 == 0 and n > 6:  # a read drawn from the span with an edit, so that real gaps get used
            cut = int(rng.integers(1, n - 3))
            read = (ref[:cut] + ref[cut + 2:])[:m] if trial % 2 else (ref[:cut] + b"T" + ref[cut:])[:m]
        else:
            read = bytes(rng.choice(alphabet, size=m).astype(np.uint8))
        assert A.best_score(ref, read, scoring, clip) == naive_best(ref, read, scoring, clip), (ref, read, scoring, clip)


def test_the_walk_and_the_grammar_on_written_out_cases():
    ref = b"AACCGGTTACGT"
    # 2 matches, a mismatch, 1I, 2 matches, 2D, 3 matches, from the third base
    nm, md, score = A.walk(ref, 3, [(3, "M"), (1, "I"), (2, "M"), (2, "D"), (3, "M")], b"CCTAGTCGT", (1, 4, 6, 1))
    assert (nm, md, score) == (4, "2G2^TA3", 7 - 4 - 7 - 8)
    # calmd's rule: D, I, D gives "^AC0^GT"; a deletion right behind a mismatch gives "0^"
    assert A.walk(b"TACGTT", 1, [(1, "M"), (2, "D"), (1, "I"), (2, "D"), (1, "M")], b"TGT", (1, 1, 0, 1))[1] == "1^AC0^GT1"
    assert A.walk(b"TACG", 1, [(1, "M"), (2, "D"), (1, "M")], b"GG", (1, 1, 0, 1))[1] == "0T0^AC1"
    good = ("50M", "2S48M", "3S20M1I10M2D14M3S", "1M")
    bad = ("2S1I47M", "47M1D2S", "1D49M", "20M2S28M", "20M30M", "0M50M", "50S", "10M5N35M", "2I48M")
    assert all(not A.grammar_errors(A.parse_cigar(c)) for c in good)
    assert all(A.grammar_errors(A.parse_cigar(c)) for c in bad) and A.parse_cigar("M50") is None
