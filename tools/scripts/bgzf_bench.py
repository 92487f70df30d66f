"""BGZF rate and ratio probe: drm_bgzf_compress_device on the BAM bytes of a simulated run of the
size sec. 4.19 used -- --lines (2,621,440) synthetic paired lines of 150 bases with AS / NM / MD tags, binned qualities
and positions uniform over --positions, encoded on the host by drm_bam_record behind drm_bam_header -- beside zlib at
levels 1 and 6 over the same 65,280-byte blocks on one host core (raw DEFLATE, so that the sizes compare payload with
payload; a member adds 26 bytes either way), and beside the host form drm_bgzf_compress, copies included. Device times are
HIP events on one stream, warm, the median of --runs runs; host times are wall clocks. Before timing, the stream is taken
apart by the reader of tests/bam_ref.py and must inflate to the input. Printed as well: the forms the members took, and
what the kernel's launch holds of a CU.
--host-only makes the bytes and runs only zlib over them, each level once as it is and once under Z_FIXED, zlib's own
fixed-Huffman form: what separates the two is what dynamic tables are worth on these bytes, whatever finds the matches.
--pipeline READS times bin/pipeline's SAM stage instead (pipeline_stage below), with and without DRM_SAM_FORMAT=bam, and
with --parent DIR beside the bin/pipeline of another checkout."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_ref  # noqa: E402
from deepreadmapper_amd import (bam_header, bam_record, bgzf_bound, bgzf_compress, bgzf_compress_device,  # noqa: E402
                                bgzf_workspace, synth)
from deepreadmapper_amd.device import DeviceBuffer, Event, Stream  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lines", type=int, default=2_621_440)
ap.add_argument("--positions", type=int, default=50_000_000)
ap.add_argument("--runs", type=int, default=11)
ap.add_argument("--zlib-stride", type=int, default=1, help="zlib takes every n-th block; its figures are scaled up")
ap.add_argument("--host-only", action="store_true",
                help="only zlib on the synthetic bytes, with the fixed-Huffman strategy as well: needs no device")
ap.add_argument("--pipeline", type=int, default=0, metavar="READS")
ap.add_argument("--parent", default="", metavar="DIR", help="with --pipeline: a checkout whose bin/pipeline runs as well")
a = ap.parse_args()
BLOCK = bam_ref.BLOCK


def pipeline_stage(n_reads, genome_len=100_000, k=32, reps=3):
    """bin/pipeline's SAM stage (DRM_SAM_STATS=1) on loci_bench.py's input: n_reads 150-base reads on a random genome
    whose first tenth is there twice, under DRM_SAM_MAPQ=1 DRM_SAM_LOCI=5 DRM_SAM_MD=1, as SAM and as BAM, each unsorted
    and sorted, `reps` times in turns; with --parent the SAM runs of that checkout's binary as well."""
    with tempfile.TemporaryDirectory() as wd:
        g = synth.genome(genome_len, seed=42)
        g = np.concatenate([g, g[:genome_len // 10]])
        fna, fq = os.path.join(wd, "g.fna"), os.path.join(wd, "reads.fastq")
        synth.write_fasta(fna, g)
        reads, names, _ = synth.simulate_reads(g, n_reads, seed=7)
        synth.write_fastq(fq, reads, names)
        subprocess.run([os.path.join(ROOT, "bin", "hnswpq_index"), fna, "idx", "150"], cwd=wd, check=True,
                       stdout=subprocess.DEVNULL)
        ways = {"sam": (ROOT, {}), "bam": (ROOT, dict(DRM_SAM_FORMAT="bam")),
                "sam sorted": (ROOT, dict(DRM_SAM_SORT="coordinate")),
                "bam sorted": (ROOT, dict(DRM_SAM_SORT="coordinate", DRM_SAM_FORMAT="bam"))}
        if a.parent:
            a.parent = os.path.abspath(a.parent)  # the runs have a working directory of their own
            ways["parent sam"] = (a.parent, {})
            ways["parent sam sorted"] = (a.parent, dict(DRM_SAM_SORT="coordinate"))
        seen = {w: [] for w in ways}
        for _ in range(reps):
            for way, (root, more) in ways.items():
                env = dict(os.environ, DRM_SAM_CIGAR="1", DRM_SAM_MAPQ="1", DRM_SAM_LOCI="5", DRM_SAM_MD="1",
                           DRM_SAM_STATS="1", **more)
                t0 = time.time()
                r = subprocess.run([os.path.join(root, "bin", "pipeline"), "idx", fq, fna, "128", str(k), str(k), "out",
                                    "1", "1"], cwd=wd, env=env, capture_output=True, text=True)
                wall = time.time() - t0
                if r.returncode != 0:
                    sys.exit(r.stdout + r.stderr)
                m = re.search(r"SAM stage: ([0-9.e+-]+) ms between the rerank and the writer, (\d+) rows aligned, "
                              r"([0-9.e+-]+) ms for the block loop", r.stdout)
                w = re.search(r"([0-9.e+-]+) ms for the final write", r.stdout)
                c = re.search(r"BAM compression: (\d+) bytes in, (\d+) bytes out, ([0-9.e+-]+) ms", r.stdout)
                out = os.path.join(wd, "out", "results.bam" if "DRM_SAM_FORMAT" in more else "results.sam")
                seen[way].append((float(m.group(1)), float(m.group(3)), float(w.group(1)) if w else 0.0, wall,
                                  os.path.getsize(out), c.groups() if c else None))
                os.remove(out)
        for way, v in seen.items():
            med = [statistics.median(x[i] for x in v) for i in range(4)]
            print(f"{way}: SAM stage {med[0]:.1f} ms, block loop {med[1]:.1f} ms, final write {med[2]:.1f} ms, process "
                  f"wall {med[3]:.2f} s (medians of {reps}); file {v[0][4]} bytes"
                  + (f"; compression {v[0][5][0]} -> {v[0][5][1]} bytes, "
                     f"{statistics.median(float(x[5][2]) for x in v):.1f} ms in drm_bgzf_compress" if v[0][5] else ""),
                  flush=True)


if a.pipeline:
    pipeline_stage(a.pipeline)
    sys.exit(0)

# ---- the run's BAM bytes
rng = np.random.default_rng(1)
N = a.lines
t0 = time.perf_counter()
text = "@HD\tVN:1.0\tSO:unsorted\n@SQ\tSN:ref\tLN:%d\n" % a.positions
pos = rng.integers(1, a.positions - 600, N // 2)
tlen = rng.integers(200, 501, N // 2)
bases = np.frombuffer(b"ACGT", dtype=np.uint8)
levels = np.frombuffer(b"#-7F", dtype=np.uint8)  # four quality bins, as recent instruments report them
parts = [bam_header(text)]
for p in range(N // 2):
    for m in range(2):
        seq = bases[rng.integers(0, 4, 150)].tobytes().decode()
        # runs of one bin, mostly the top one
        q = np.repeat(rng.choice(4, size=12, p=(0.04, 0.08, 0.18, 0.7)), rng.multinomial(150, np.full(12, 1 / 12)))
        nm = int(rng.integers(0, 3))
        md = "150" if nm == 0 else "70A79" if nm == 1 else "30C50G68"
        here, there = (pos[p], pos[p] + tlen[p] - 150) if m == 0 else (pos[p] + tlen[p] - 150, pos[p])
        line = (f"read{p}\t{(99, 147)[m]}\tref\t{here}\t{int(rng.integers(0, 61))}\t150M\t=\t{there}\t"
                f"{tlen[p] if m == 0 else -tlen[p]}\t{seq}\t{levels[q].tobytes().decode()}\tAS:i:{150 - 5 * nm}\tNM:i:{nm}"
                f"\tMD:Z:{md}")
        parts.append(bam_record(line, ["ref"]))
data = b"".join(parts)
del parts
n = len(data)
blocks = -(-n // BLOCK)
print(f"{N} lines -> {n} BAM bytes, {blocks} blocks ({time.perf_counter() - t0:.1f} s to make them); workspace "
      f"{bgzf_workspace(n) / 2 ** 20:.0f} MiB", flush=True)



def zlib_blocks(level, strategy):
    """(bytes with the members' 26 each, seconds) of raw DEFLATE per block on this core, scaled up from every
    --zlib-stride-th block."""
    total, t0 = 0, time.perf_counter()
    taken = range(0, blocks, a.zlib_stride)
    for b in taken:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        total += len(c.compress(data[b * BLOCK:(b + 1) * BLOCK])) + len(c.flush())
    return total * blocks / len(taken) + 26 * blocks, (time.perf_counter() - t0) * blocks / len(taken)


if a.host_only:
    for level in (1, 6):
        for name, strategy in (("default strategy", zlib.Z_DEFAULT_STRATEGY), ("Z_FIXED", zlib.Z_FIXED)):
            size, sec = zlib_blocks(level, strategy)
            print(f"zlib level {level}, {name}: {size:.0f} bytes = {size / n:.4f} of the input, {sec:.1f} s", flush=True)
    sys.exit(0)

# ---- the stream, checked
st = Stream()
d_data = DeviceBuffer.from_host(np.frombuffer(data, dtype=np.uint8))
d_out, d_sizes = DeviceBuffer((bgzf_bound(n),), np.uint8), DeviceBuffer((blocks,), np.uint32)
work = DeviceBuffer((bgzf_workspace(n),), np.uint8)


def ours():
    bgzf_compress_device(d_data, n, d_out, d_sizes, st, work)


ours()
st.synchronize()
sizes = d_sizes.download()
stream = d_out.download()[:int(sizes.sum())].tobytes()
raw, btypes, _ = bam_ref.read_bgzf(stream, eof=False)
assert raw == data
print(f"drm_bgzf_compress_device: {len(stream)} bytes = {len(stream) / n:.4f} of the input ({n / len(stream):.3f} : 1); "
      f"{btypes.count(1)} members fixed Huffman, {btypes.count(0)} stored; the reader inflates it to the input", flush=True)


def timed(f):
    e0, e1 = Event(), Event()
    e0.record(st)
    f()
    e1.record(st)
    st.synchronize()
    return e0.elapsed_ms(e1)


for _ in range(2):
    ours()
st.synchronize()
t = [timed(ours) for _ in range(a.runs)]
m = statistics.median(t)
print(f"drm_bgzf_compress_device: median {m:.3f} ms (min {min(t):.3f}, max {max(t):.3f}, {len(t)} runs) = "
      f"{n / (m * 1e-3) / 1e9:.2f} GB/s of input, {m * 1e3 / blocks:.2f} us a block over the whole call", flush=True)
cus = 256
print(f"  one workgroup of 1024 lanes a CU (its LDS, 139.6 KiB of 160, allows no second): 16 waves a CU, 4 a SIMD; {blocks} "
      f"blocks on {cus} CUs = {blocks / cus:.1f} blocks a CU, {m * 1e3 / (blocks / cus):.1f} us a block and CU", flush=True)

# ---- the host form, copies included
t = []
for _ in range(3):
    t0 = time.perf_counter()
    got = bgzf_compress(data)
    t.append((time.perf_counter() - t0) * 1e3)
assert got == stream
mh = statistics.median(t)
print(f"drm_bgzf_compress (host memory in and out, pinned staging, rounds of 256 blocks): median {mh:.1f} ms of 3 = "
      f"{n / (mh * 1e-3) / 1e9:.2f} GB/s; the same stream", flush=True)

# ---- zlib on one host core over the same blocks
for level in (1, 6):
    size, sec = zlib_blocks(level, zlib.Z_DEFAULT_STRATEGY)
    taken = range(0, blocks, a.zlib_stride)
    print(f"zlib level {level}, one core, {len(taken)} of {blocks} blocks: {size:.0f} bytes with the members' 26 each = "
          f"{size / n:.4f} of the input ({n / size:.3f} : 1), {sec:.1f} s = {n / sec / 1e6:.0f} MB/s; ours is "
          f"{len(stream) / size:.3f} of its size in {m * 1e-3 / sec:.6f} of its time", flush=True)
