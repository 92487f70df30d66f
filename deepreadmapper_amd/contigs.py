"""Multi-contig references: the contig table of a FASTA in the coordinates of extract_fasta_sequence's string
(drm_fasta_contigs), the table on a device with its host lookup (drm_contigs_create / drm_contigs_find), and the GPU
stage that keeps the rerank rows whose window lies inside one contig and gives them spread ids (drm_contig_hits, the
HIP kernel of csrc/contig_hits.hip). The definitions are in include/drm_hip.h."""
import ctypes as C

import numpy as np

from ._native import check, lib, ptr
from .pairing import _rows

CONTIG_SHIFT = 33  # spread id = id + (contig << 33): the position shifted by contig * 2^32


def fasta_contigs(path):
    """drm_fasta_contigs: (names, starts, lens) of the FASTA's contigs -- a list of str and two int64 arrays -- such
    that extract_fasta_sequence(path)[starts[t] : starts[t] + lens[t]] is contig t's sequence."""
    n, nb = C.c_int64(0), C.c_int64(0)
    p = str(path).encode()
    check(lib().drm_fasta_contigs(p, C.byref(n), None, None, None, C.byref(nb)))
    starts, lens = np.zeros(n.value, dtype=np.int64), np.zeros(n.value, dtype=np.int64)
    names = C.create_string_buffer(max(nb.value, 1))
    check(lib().drm_fasta_contigs(p, C.byref(n), ptr(starts), ptr(lens), names, C.byref(nb)))
    return [s.decode() for s in names.raw[:nb.value].split(b"\0")[:n.value]], starts, lens


def lds_max():
    """drm_contig_lds_max: the largest table contig_hits searches in LDS."""
    return int(lib().drm_contig_lds_max())


class ContigTable:
    """A contig table on a device (drm_contigs): starts and lens in the genome string's coordinates, ascending and
    disjoint. `names` is kept for the caller."""

    def __init__(self, starts, lens, device=0, names=None):
        self.starts = np.ascontiguousarray(starts, dtype=np.int64)
        self.lens = np.ascontiguousarray(lens, dtype=np.int64)
        if self.starts.ndim != 1 or self.starts.shape != self.lens.shape:
            raise ValueError("starts and lens must be 1-d arrays of one length")
        self.names = None if names is None else list(names)
        self.device = int(device)
        self.handle = C.c_void_p()
        check(lib().drm_contigs_create(ptr(self.starts), ptr(self.lens), len(self.starts), self.device,
                                       C.byref(self.handle)))

    @classmethod
    def from_fasta(cls, path, device=0):
        names, starts, lens = fasta_contigs(path)
        return cls(starts, lens, device, names)

    def __len__(self):
        return len(self.starts)

    def find(self, pos, span=0):
        """drm_contigs_find: the contig that contains [pos, pos + span) wholly, or -1. Host only."""
        t = C.c_int32(-1)
        check(lib().drm_contigs_find(self.handle, int(pos), int(span), C.byref(t)))
        return t.value

    def free(self):
        if self.handle:
            check(lib().drm_contigs_free(self.handle))
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def contig_hits(table, ids, scores, cnt, ref_len):
    """drm_contig_hits on host arrays: ids [reads, k] u64 window ids, scores [reads, k] i32 and cnt [reads] i32 of a
    rerank output. Returns (out_ids, out_spread, out_scores, out_contig, out_cnt): each read's rows whose window lies
    inside one contig, in their order, their spread ids id + (contig << 33), scores and contigs, and the number kept;
    the rows behind them hold 2^64 - 1, 2^64 - 1, 0 and -1."""
    i, s = _rows(ids, np.uint64), _rows(scores, np.int32)
    c = np.ascontiguousarray(cnt, dtype=np.int32)
    if not (i.ndim == 2 and i.shape == s.shape and c.shape == (len(i),)):
        raise ValueError("ids, scores [reads, k] and cnt [reads] must agree")
    oi, osp = np.zeros_like(i), np.zeros_like(i)
    osc, oc = np.zeros_like(s), np.zeros_like(s)
    ocnt = np.zeros_like(c)

    def p(a):
        return ptr(a) if a.size else None
    check(lib().drm_contig_hits(table.handle, int(ref_len), p(i), p(s), ptr(c), len(c), int(i.shape[1]), p(oi), p(osp),
                                p(osc), p(oc), ptr(ocnt)))
    return oi, osp, osc, oc, ocnt


def contig_hits_device(table, d_ids, d_scores, d_cnt, nreads, k, ref_len, d_out=None, stream=None):
    """drm_contig_hits_device: the same on device memory, enqueued on `stream`. Each d_* argument is a DeviceBuffer or a
    raw device address; d_out is the tuple of the five output buffers (new ones when None). Returns that tuple;
    synchronise the stream before downloading."""
    from .device import DeviceBuffer

    def addr(b):
        return None if b is None else C.c_void_p(b.ptr if hasattr(b, "ptr") else int(b))
    if d_out is None:
        shape = (int(nreads), int(k))
        d_out = (DeviceBuffer(shape, np.uint64), DeviceBuffer(shape, np.uint64), DeviceBuffer(shape, np.int32),
                 DeviceBuffer(shape, np.int32), DeviceBuffer((int(nreads),), np.int32))
    check(lib().drm_contig_hits_device(table.handle, int(ref_len), addr(d_ids), addr(d_scores), addr(d_cnt),
                                       int(nreads), int(k), *[addr(b) for b in d_out],
                                       stream.handle if stream is not None else None))
    return d_out
