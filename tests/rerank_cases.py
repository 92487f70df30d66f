"""Windows, reads, candidate lists and the fixed cases shared by tests/test_gpu_rerank_dispatch.py and the child
process it starts (tests/sw_bitprofile_child.py).

Reads are built as `test_gpu_sw_pairadd._reads_from` builds them (cut from the windows, some with a few substitutions,
every fifth one unrelated), one read at a time so that a batch can mix lengths."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
N_DNA, N_ALPHA = 48, 16  # DNA windows, then windows over a 40-letter alphabet


def dna(rng, *shape):
    return rng.choice(ACGT, size=shape).astype(np.uint8)


def alpha(rng, *shape):
    """bytes 33..72: 40 letters, A, C and G among them"""
    return rng.integers(33, 73, size=shape).astype(np.uint8)


def windows(rng, length, n_dna=N_DNA, n_alpha=N_ALPHA):
    if not n_alpha:
        return dna(rng, n_dna, length)
    return np.concatenate([dna(rng, n_dna, length), alpha(rng, n_alpha, length)])


def cut(rng, w, cols, fill):
    """`cols` bytes cut from window w; a window shorter than that is held whole inside bytes from `fill`"""
    if len(w) < cols:
        o = int(rng.integers(0, cols - len(w) + 1))
        r = fill(rng, cols)
        r[o:o + len(w)] = w
        return r
    o = int(rng.integers(0, len(w) - cols + 1))
    return w[o:o + cols].copy()


def dna_read(rng, refs, i, cols, tags, n_dna=N_DNA):
    """read i of a batch: `cols` bases of DNA window i % n_dna (i % 3 == 1: a few substitutions; i % 5 == 4:
    unrelated), tagged like format_fastq when asked. Returns (read, its window)."""
    own = i % n_dna
    if i % 5 == 4:
        r = dna(rng, cols)
    else:
        r = cut(rng, refs[own], cols, dna)
        if i % 3 == 1 and len(refs[own]) >= cols:
            for p in rng.integers(0, cols, size=max(1, cols // 20)):
                r[p] = ACGT[(int(np.searchsorted(ACGT, r[p])) + 1) % 4]
    return (b"<" + bytes(r) + b">") if tags else bytes(r), own


def byte_reads(rng, refs, lengths, n_dna=N_DNA):
    """One read per entry of `lengths` (its length in BYTES): every third one over the 40-letter alphabet, cut from an
    alphabet window; the others DNA, odd ones tagged ("<" + n - 2 bases + ">": n - 2 DP columns on the class-profile
    path), even ones untagged (n columns). Returns (reads, own windows)."""
    reads, own = [], []
    n_alpha = len(refs) - n_dna
    for i, n in enumerate(lengths):
        n = int(n)
        if i % 3 == 2 and n_alpha:
            w = n_dna + i % n_alpha
            reads.append(bytes(cut(rng, refs[w], n, alpha)))
            own.append(w)
        else:
            tags = i % 2 == 1 and n >= 3
            r, w = dna_read(rng, refs, i, n - 2 * tags, tags, n_dna)
            reads.append(r)
            own.append(w)
    return reads, np.array(own, np.int64)


def lists(rng, own, n_ref, ncand):
    """candidate lists: the read's own window first, then random ones (repeats allowed, as the search may give)"""
    nb = rng.integers(0, n_ref, size=(len(own), ncand)).astype(np.int64)
    nb[:, 0] = own
    return nb


def dense_lists(rng, own, n_ref, ncand, n_bad):
    """lists of `ncand` in-range ids (repeats among them) with `n_bad` out-of-range ids strewn in, which are dropped"""
    nq = len(own)
    nb = np.empty((nq, ncand + n_bad), np.int64)
    bad = np.array([-1, n_ref, n_ref + 5, 1 << 40, -(1 << 33), n_ref + (1 << 32), 1 << 62], np.int64)
    for q in range(nq):
        row = rng.integers(0, n_ref, size=ncand).astype(np.int64)
        row[0] = own[q]
        at = np.sort(rng.choice(ncand + n_bad, size=n_bad, replace=False))
        keep = np.ones(ncand + n_bad, bool)
        keep[at] = False
        nb[q, keep] = row
        nb[q, at] = bad[np.arange(n_bad) % len(bad)]
    return nb


def cases():
    """The bit-profile child's cases, (name, windows, lists, reads, stride, k, k_clusters): reads of 40, 150 and 152
    bytes, tagged (38 / 148 / 150 DP columns between the tags) and untagged, every third read over the 40-letter
    alphabet, one batch of mixed lengths, windows of 150 and of 161 bytes, and lists of 1024 candidates for the <64> and
    the <152> instantiation."""
    out = []
    for qlen, wlen in ((40, 150), (150, 150), (152, 150), (152, 161), (64, 161)):
        rng = np.random.default_rng(8000 + 10 * qlen + wlen)
        refs = windows(rng, wlen)
        reads, own = byte_reads(rng, refs, [qlen] * 24)
        out.append((f"q{qlen}_w{wlen}", refs, lists(rng, own, len(refs), 72), reads, 1, 72, 72))
    rng = np.random.default_rng(8500)
    refs = windows(rng, 150)
    lengths = rng.integers(3, 153, size=24)
    lengths[5] = 152
    reads, own = byte_reads(rng, refs, lengths)
    out.append(("mixed_to_152", refs, lists(rng, own, len(refs), 72), reads, 1, 5, 72))
    for qlen in (42, 152):
        rng = np.random.default_rng(8600 + qlen)
        refs = windows(rng, 150)
        reads, own = byte_reads(rng, refs, [qlen] * 8)
        out.append((f"c1024_q{qlen}", refs, dense_lists(rng, own, len(refs), 1024, 0), reads, 1, 1024, 1024))
        out.append((f"c1024_q{qlen}_k5", refs, dense_lists(rng, own, len(refs), 1017, 7), reads, 1, 5, 1024))
    return out
