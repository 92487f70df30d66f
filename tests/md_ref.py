"""Plain Python restatement of the MD words and the MD:Z string defined in include/drm_hip.h (drm_sw_align_md,
drm_sam_md) -- a helper for the tests, not a test. The reference prints no tags, so this file is what the GPU
result must equal on every pair. rebuild_reference is independent of the first two functions: it reads a printed
SEQ, CIGAR and MD the way a consumer of the SAM line does."""
import re

from sw_align_ref import D, I, M

MD_FIELDS = ("n_words", "n_match", "n_mismatch", "n_ins", "n_del", "status")
NUMBER, MISMATCH, DELETED = 0, 1, 2
MAX_OPS = 512
_COMP = {ord(a): ord(b) for a, b in zip("ATCGN", "TAGCN")}


def _empty(status):
    return dict.fromkeys(MD_FIELDS, 0) | {"status": status}, []


def md_words(region, query, record, ops):
    """(md record dict, list of words) for one pair: `region` and `query` the bytes the aligner saw, `record` its
    drm_sw_alignment (a mapping or a structured row), `ops` the operation words of the pair."""
    region, query = bytes(region), bytes(query)
    r = {f: int(record[f]) for f in ("ref_begin", "ref_end", "q_begin", "q_end", "n_ops", "status")}
    if r["status"] == 1 or not region or not query:
        return _empty(1)
    if r["status"] != 0 or not 1 <= r["n_ops"] <= MAX_OPS:
        return _empty(3)
    if r["ref_begin"] < 0 or r["q_begin"] < 0 or r["ref_begin"] > r["ref_end"] or r["ref_end"] > len(region) \
            or r["q_end"] > len(query):
        return _empty(3)
    words = [int(x) for x in ops[:r["n_ops"]]]
    assert len(words) == r["n_ops"], "the caller passes every word the record counts"
    if any((w & 15) > 2 or (w >> 4) == 0 for w in words):
        return _empty(3)
    if sum(w >> 4 for w in words if (w & 15) != I) != r["ref_end"] - r["ref_begin"] \
            or sum(w >> 4 for w in words if (w & 15) != D) != r["q_end"] - r["q_begin"]:
        return _empty(3)
    out, run = [], 0
    i, j = r["ref_begin"], r["q_begin"]
    n_match = n_mismatch = n_ins = n_del = 0
    for w in words:
        n, op = w >> 4, w & 15
        if op == M:
            for _ in range(n):
                if region[i] == query[j]:
                    run += 1
                    n_match += 1
                else:
                    out += [(run << 4) | NUMBER, (region[i] << 4) | MISMATCH]
                    run = 0
                    n_mismatch += 1
                i, j = i + 1, j + 1
        elif op == I:
            j += n
            n_ins += n
        else:
            out.append((run << 4) | NUMBER)
            run = 0
            out += [(region[i + x] << 4) | DELETED for x in range(n)]
            i += n
            n_del += n
    out.append((run << 4) | NUMBER)
    return {"n_words": len(out), "n_match": n_match, "n_mismatch": n_mismatch, "n_ins": n_ins, "n_del": n_del,
            "status": 0}, out


def md_string(words, reverse):
    """The MD:Z string of a complete word list by drm_sam_md's rules; ValueError where it returns DRM_ERR_ARG."""
    words = [int(w) for w in words]
    if reverse:
        words = words[::-1]
    if not words or (words[0] & 15) != NUMBER or (words[-1] & 15) != NUMBER:
        raise ValueError("an MD stream starts and ends with a number")
    s, prev = "", None
    for w in words:
        kind, value = w & 15, w >> 4
        if kind > 2:
            raise ValueError("kind")
        if kind == NUMBER:
            if prev == NUMBER:
                raise ValueError("two numbers")
            s += str(value)
        else:
            base = _COMP.get(value, 0) if reverse else value
            if not ord("A") <= base <= ord("Z"):
                raise ValueError("base")
            if kind == DELETED and prev != DELETED:
                s += "^"
            s += chr(base)
        prev = kind
    return s


def rebuild_reference(seq, cigar, md):
    """The reference bytes under the alignment of a SAM line, from its printed SEQ, CIGAR and MD alone."""
    seq = seq.encode() if isinstance(seq, str) else bytes(seq)
    # the read bases of the M columns, None where the column is a deletion
    cols, at = [], 0
    for n, op in re.findall(r"(\d+)([MIDS])", cigar):
        n = int(n)
        if op == "M":
            cols += [seq[at + x] for x in range(n)]
        if op == "D":
            cols += [None] * n
        if op in "MIS":
            at += n
    assert at == len(seq), "the CIGAR does not span SEQ"
    assert re.fullmatch(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*", md), md
    out, c = [], 0
    for num, sub, dele in re.findall(r"([0-9]+)|([A-Z])|\^([A-Z]+)", md):
        if num:
            for _ in range(int(num)):
                assert cols[c] is not None, "MD counts a match on a deleted column"
                out.append(cols[c])
                c += 1
        elif sub:
            assert cols[c] is not None and cols[c] != ord(sub), "an MD mismatch equals the read base"
            out.append(ord(sub))
            c += 1
        else:
            for ch in dele:
                assert cols[c] is None, "MD deletes a column the CIGAR aligns"
                out.append(ord(ch))
                c += 1
    assert c == len(cols), "MD and CIGAR cover different numbers of reference bases"
    return bytes(out)


def nm_from_cigar_md(cigar, md):
    """Edit distance of a SAM line: mismatch letters of MD plus the I and D bases of the CIGAR."""
    indel = sum(int(n) for n, op in re.findall(r"(\d+)([MIDS])", cigar) if op in "ID")
    return indel + len(re.findall(r"[A-Z]", re.sub(r"\^[A-Z]+", "^", md)))
