// Popped ties in the wave heap (tools/emu/wave_emu.h) against a literal faiss MinimaxHeap: a heap slot's key keeps its
// node id when pop_min takes it (bit 31 of the low word cleared), where faiss writes id -1, so two popped slots of one
// distance are equal to faiss and differ in the raw keys; the wave heap compares through N wherever both sides can be
// popped. The sequences here make such ties decide sift-downs: 1 - 3 distinct distances fill the heap, pop_min takes
// between none and all of the slots, then every push lies strictly below the root (a full-heap replace: heap_pop of
// the last slot from the root, then heap_push), some with further pop_mins between them. Heaps of 128 slots run
// replace128 / push_fill, heaps of 2 - 127 slots the general pop / push. After every step all slots' keys and nodes,
// the root and holds() of every id used so far are compared with the literal heap.
// The literal heap counts, inside its sift-downs, the compares that the layout could get wrong:
//   (i)   both children popped, equal distance;
//   (ii)  the sifted last slot popped, against a popped child of equal distance (another slot than itself);
//   (iii) a popped and a live operand of equal distance: popped first, and live first.
// Output: "ok: ..." and one "counts <path> i ii iii_popped_live iii_live_popped" line per path (full128, general).
// Test infrastructure (tests/test_heap_model_popped_ties.py): g++ -O2 -std=c++17 heap_ties_emu.cpp -o heap_ties_emu
#include "wave_emu.h"

struct Counts { long i = 0, ii = 0, pl = 0, lp = 0; };

// literal faiss MinimaxHeap (0-based arrays, 1-based algorithms) with the node of every slot kept aside
struct Ref {
    int n, k = 0;
    std::vector<u32> dis; std::vector<int32_t> ids, node;
    Counts *cnt;
    Ref(int n_, Counts *c) : n(n_), dis(n_), ids(n_), node(n_), cnt(c) {}
    static bool cmp2(u32 a1, u32 b1, int32_t a2, int32_t b2) { return a1 > b1 || (a1 == b1 && a2 > b2); }
    void tally_mixed(u32 a1, u32 b1, int32_t a2, int32_t b2) {
        if (a1 != b1) return;
        if (a2 == -1 && b2 != -1) ++cnt->pl;
        if (a2 != -1 && b2 == -1) ++cnt->lp;
    }
    void heap_pop(int kk) {
        u32 *bv = dis.data() - 1; int32_t *bi = ids.data() - 1, *bn = node.data() - 1;
        const u32 v = bv[kk]; const int32_t id = bi[kk];
        int i = 1;
        for (;;) {
            const int i1 = i << 1, i2 = i1 + 1;
            if (i1 > kk) break;
            bool left = i2 == kk + 1;
            if (!left) {
                if (bv[i1] == bv[i2] && bi[i1] == -1 && bi[i2] == -1) ++cnt->i;
                tally_mixed(bv[i1], bv[i2], bi[i1], bi[i2]);
                left = cmp2(bv[i1], bv[i2], bi[i1], bi[i2]);
            }
            const int c = left ? i1 : i2;
            if (c != kk) {
                if (v == bv[c] && id == -1 && bi[c] == -1) ++cnt->ii;
                tally_mixed(v, bv[c], id, bi[c]);
            }
            if (cmp2(v, bv[c], id, bi[c])) break;
            bv[i] = bv[c]; bi[i] = bi[c]; bn[i] = bn[c]; i = c;
        }
        bv[i] = bv[kk]; bi[i] = bi[kk]; bn[i] = bn[kk];
    }
    void heap_push(int kk, u32 v, int32_t id) {
        u32 *bv = dis.data() - 1; int32_t *bi = ids.data() - 1, *bn = node.data() - 1;
        int i = kk;
        while (i > 1) { const int f = i >> 1; if (!cmp2(v, bv[f], id, bi[f])) break; bv[i] = bv[f]; bi[i] = bi[f]; bn[i] = bn[f]; i = f; }
        bv[i] = v; bi[i] = id; bn[i] = id;
    }
    bool push(int32_t i, u32 v) {
        if (k == n) { if (v >= dis[0]) return false; heap_pop(k--); }
        heap_push(++k, v, i); return true;
    }
    int pop_min() { // the slot taken: the smallest valid one, the highest index among ties; -1: none valid
        int i = k - 1; while (i >= 0 && ids[i] == -1) --i;
        if (i < 0) return -1;
        int imin = i; u32 vmin = dis[i];
        for (--i; i >= 0; --i) if (ids[i] != -1 && dis[i] < vmin) { vmin = dis[i]; imin = i; }
        ids[imin] = -1; return imin;
    }
};

static u64 &slot(Heap &h, int s) { if (s == 0) return h.R[63]; const int o = (s - 1) >> 1; return (s & 1) ? h.L[o] : h.R[o]; }

static void fail(const char *what, int t, int step) { std::printf("trial %d step %d: %s\n", t, step, what); std::exit(1); }

int main(int argc, char **argv)
{
    const int trials = argc > 1 ? std::atoi(argv[1]) : 400;
    const PathConst pc;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 11);
    Counts full, general;
    long checks = 0, replaces = 0;
    for (int t = 0; t < trials; ++t) {
        // every other trial a smaller heap: the general pop / push path. Sizes 2 .. 127, each reached in turn
        const int n = (t & 1) ? 2 + (t >> 1) % 126 : 128;
        Counts &cnt = n == 128 ? full : general;
        Heap hp; hp.init();
        Ref ref(n, &cnt);
        const int nd = 1 + (int)(rng() % 3);          // distinct distances of the fill
        const int nlow = 1 + (int)(rng() % 3);        // and of the pushes below it
        const u32 base = 0x80000100u;                 // ord32 keys of non-negative distances have bit 31 set
        int32_t next_id = 0; int kc = 0, step = 0;
        auto check = [&]() {
            for (int s = 0; s < ref.k; ++s) {
                // faiss's key (a popped slot's id is -1) is the slot's key through N; the raw key keeps the node
                const u64 want = ((u64)ref.dis[s] << 32) | (u32)((u32)ref.ids[s] ^ kLive);
                const u64 raw = ((u64)ref.dis[s] << 32) | ((u32)ref.node[s] | (ref.ids[s] == -1 ? 0u : kLive));
                const u64 got = slot(hp, s);
                if (normk(got) != want || got != raw || node_of(got) != ref.node[s] || is_live(got) != (ref.ids[s] != -1)) {
                    std::printf("trial %d (n %d) step %d slot %d: key %016llx, want %016llx (faiss's %016llx)\n", t, n, step, s,
                                (unsigned long long)got, (unsigned long long)raw, (unsigned long long)want);
                    std::exit(1);
                }
                ++checks;
            }
            for (int s = ref.k; s < 128; ++s) if (slot(hp, s) != kUnused) fail("a slot past the heap's size was written", t, step);
            for (int32_t v = 0; v <= next_id; ++v) { // next_id itself: never pushed
                bool in_ref = false;
                for (int s = 0; s < ref.k; ++s) in_ref |= ref.node[s] == v;
                if (hp.holds(v) != in_ref) fail("holds() differs from the literal heap's nodes", t, step);
            }
            ++step;
        };
        auto push = [&](u32 key) { // as the kernel pushes: fill, or replace when the key lies below the full heap's root
            const int32_t id = next_id++;
            const bool full_heap = kc == n;
            if (full_heap && key >= hi32(hp.R[63])) fail("push at or above the root", t, step);
            if (!ref.push(id, key)) fail("the literal heap rejected the push", t, step);
            if (kc == 0) { hp.R[63] = pack(key, id); kc = 1; }
            else if (full_heap) {
                ++replaces;
                if (n == 128) { if (hp.replace128(pack(key, id), pc) != hp.R[63]) fail("replace128's root", t, step); }
                else { hp.pop(kc); hp.push(kc, pack(key, id)); }
            } else if (n == 128) hp.push_fill(++kc, pack(key, id), pc);
            else hp.push(++kc, pack(key, id));
            check();
        };
        auto pop_min = [&]() {
            const int s = ref.pop_min();
            if (s < 0) return;
            slot(hp, s) = mark_popped(slot(hp, s)); // pop_min's marking: bit 31 of the low word cleared
            check();
        };
        for (int j = 0; j < n; ++j) push(base + (u32)(rng() % nd));
        const int npop = (int)(rng() % (n + 1)); // between none and all of the slots
        for (int j = 0; j < npop; ++j) pop_min();
        const bool interleave = rng() & 1;
        // pushes strictly below the root: nlow distances below every fill distance, while the root is a fill entry --
        // at most n of them, fewer when the root falls into the low band
        for (int j = 0; j < n; ++j) {
            const u32 key = base - 1u - (u32)(rng() % nlow);
            if (key >= hi32(hp.R[63])) break;
            push(key);
            if (interleave && rng() % 3 == 0) pop_min();
        }
    }
    std::printf("ok: %d trials, %ld replaces, %ld slot checks\n", trials, replaces, checks);
    std::printf("counts full128 %ld %ld %ld %ld\n", full.i, full.ii, full.pl, full.lp);
    std::printf("counts general %ld %ld %ld %ld\n", general.i, general.ii, general.pl, general.lp);
    return 0;
}
