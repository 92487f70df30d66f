"""Plain Python / numpy restatements of the multi-contig definitions of include/drm_hip.h: the contig table of a FASTA
(drm_fasta_contigs), the host lookup (drm_contigs_find) and the contig stage (drm_contig_hits)."""
import numpy as np

BASES = b"ACGTN"
FILL = np.uint64(2**64 - 1)
SHIFT = 33


class FormatError(ValueError):
    """What drm_fasta_contigs answers with DRM_ERR_FORMAT; `.contig` is the index of the contig it names."""

    def __init__(self, contig, what):
        super().__init__(f"contig {contig}: {what}")
        self.contig = contig


def extract(data):
    """drm_extract_fasta_sequence: skip the first line, keep the upper-cased A/C/G/T/N of everything after it."""
    nl = data.find(b"\n")
    rest = b"" if nl < 0 else data[nl + 1:]
    return bytes(c for c in rest.upper() if c in BASES)


def fasta_contigs(data):
    """(names, starts, lens) of the FASTA text `data` (bytes), or FormatError."""
    if not data.startswith(b">"):
        raise FormatError(0, "the first line is no header")
    names, starts, lens = [], [], []
    glen = 0

    def close():
        lens.append(glen - starts[-1])
        if lens[-1] == 0:
            raise FormatError(len(names) - 1, "no sequence")
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()  # the text after the last newline, when there is none
    for line in lines:
        if line.startswith(b">"):
            if names:
                close()
                glen += sum(c in BASES for c in line.upper())
            name = line[1:].split(b" ")[0].split(b"\t")[0].split(b"\r")[0].split(b"\v")[0].split(b"\f")[0].decode()
            if not name:
                raise FormatError(len(names), "empty name")
            if name in names:
                raise FormatError(len(names), "duplicate name")
            names.append(name)
            starts.append(glen)
        else:
            for c in line:
                if c in b" \t\n\v\f\r":
                    continue
                if bytes([c]).upper()[0] not in BASES:
                    raise FormatError(len(names) - 1, f"byte {chr(c)!r} would be dropped")
                glen += 1
    close()
    return names, np.array(starts, dtype=np.int64), np.array(lens, dtype=np.int64)


def find(starts, lens, pos, span):
    """drm_contigs_find: the contig holding [pos, pos + span) wholly, or -1."""
    if pos < 0 or span < 0:
        return -1
    for t in reversed(range(len(starts))):  # the last contig that starts at or before pos decides (span 0 at a seam)
        if int(starts[t]) <= pos:
            return t if pos + span <= int(starts[t]) + int(lens[t]) else -1
    return -1


def contig_hits(starts, lens, ids, scores, cnt, ref_len):
    """drm_contig_hits: (out_ids, out_spread, out_scores, out_contig, out_cnt)."""
    ids = np.asarray(ids, dtype=np.uint64)
    scores = np.asarray(scores, dtype=np.int32)
    nreads, k = ids.shape
    st = np.asarray(starts, dtype=np.uint64)
    en = st + np.asarray(lens, dtype=np.uint64)
    p = ids >> np.uint64(1)
    t = np.searchsorted(st, p.ravel(), side="right").reshape(p.shape).astype(np.int64) - 1  # the last start <= p
    tc = np.maximum(t, 0)
    counted = np.arange(k)[None, :] < np.clip(np.asarray(cnt, dtype=np.int64), 0, k)[:, None]
    keep = counted & (t >= 0) & (p + np.uint64(ref_len) <= en[tc])  # p < 2^63: the sum does not wrap
    out_ids = np.full((nreads, k), FILL, dtype=np.uint64)
    out_spread = np.full((nreads, k), FILL, dtype=np.uint64)
    out_scores = np.zeros((nreads, k), dtype=np.int32)
    out_contig = np.full((nreads, k), -1, dtype=np.int32)
    out_cnt = keep.sum(axis=1).astype(np.int32)
    order = np.argsort(~keep, axis=1, kind="stable")  # kept rows first, in their order
    dst = np.arange(k)[None, :] < out_cnt[:, None]
    src_ids = np.take_along_axis(ids, order, axis=1)
    src_t = np.take_along_axis(tc, order, axis=1)
    out_ids[dst] = src_ids[dst]
    out_spread[dst] = src_ids[dst] + (src_t[dst].astype(np.uint64) << np.uint64(SHIFT))
    out_scores[dst] = np.take_along_axis(scores, order, axis=1)[dst]
    out_contig[dst] = src_t[dst].astype(np.int32)
    return out_ids, out_spread, out_scores, out_contig, out_cnt
