"""Popped ties in the host model of the lean search kernel's heap (tools/emu/wave_emu.h, driven by
tools/emu/heap_ties_emu.cpp) against a literal faiss MinimaxHeap. A heap slot's key keeps its node id when pop_min
takes it (bit 31 of the low word cleared) where faiss writes id -1; the heap compares through N(w) = max(w, 2^31 - 1)
wherever both operands can be popped, so that two popped slots of one distance stay equal as they are to faiss.
The driver fills heaps of 128 slots (replace128 / push_fill) and of every size 2 .. 127 (the general pop / push)
with 1 - 3 distinct distances, pops between none and all of the slots and then pushes strictly below the root,
comparing every slot's key and node, the root and holds() after every step. CPU only.

The literal heap counts the compares inside its sift-downs that the layout could get wrong: (i) both children popped
with equal distance, (ii) the sifted last slot popped against a popped child of equal distance, (iii) a popped and
a live operand of equal distance, either way round. A run in which one of them never happened proves nothing about
it, so each count must be positive, on the 128-slot path and on the general one."""
import os
import subprocess

from conftest import ROOT

EMU = os.path.join(ROOT, "tools", "emu")


def test_popped_ties_decide_sifts_as_in_faiss(tmp_path):
    exe = str(tmp_path / "heap_ties_emu")
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(EMU, "heap_ties_emu.cpp"), "-o", exe], check=True)
    # 400 trials: 200 full heaps, and every size 2 .. 127 of the general path at least once (about 1 s)
    r = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), r.stdout + r.stderr
    counts = {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "counts":
            counts[w[1]] = dict(zip(["both_children_popped_equal", "last_slot_and_child_popped_equal",
                                     "popped_vs_live_equal", "live_vs_popped_equal"], map(int, w[2:])))
    print(counts)
    assert set(counts) == {"full128", "general"}, r.stdout
    for path, c in counts.items():
        for what, v in c.items():
            assert v > 0, f"{path}: no sift-down met the case {what} ({c})"
