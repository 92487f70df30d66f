// deepreadmapper_amd/csrc/sort_order.hip -- the stable sort of the SAM lines' keys, for gfx950.
//
// drm_sort_order (include/drm_hip.h): order[i] = the input index of the key that comes i-th, equal keys in input order.
// A least-significant-digit radix sort over the eight bytes of a key that carries the key's input index as a uint32
// payload. Everything is enqueued on one stream and nothing comes back to the host in between:
// which passes run is decided on the device.
//
//   histogram  one pass over the keys: hist[p][v] = the keys whose byte p is v, for all eight p. Per block the counts are
//              collected in LDS and added to the global table by vector atomics; a count does not depend on the order of
//              its additions, so this, and the count below, are the places where atomics are used.
//              The same pass counts the all-ones keys (the lines without RNAME), hist[kSortOnes].
//   plan       one block. Pass p is dropped when one value holds all n keys (a byte that is the same in every key cannot
//              change the order). It is also dropped when byte p only tells the all-ones keys from the rest -- its value
//              255 holds exactly the all-ones keys and one other value holds every other key -- and a lower byte that
//              does the same is kept: an all-ones key is the largest in every byte, so one such pass, wherever it
//              stands, puts those keys behind all others, and a second one changes nothing. Real keys use four or five
//              bytes, and without this rule two per cent of unmapped lines would keep all eight passes alive.
//              The kept passes, in order, get their buffers: keys d_keys -> K0 -> K1 -> K0 ..., the
//              last kept pass writing no keys; payloads (iota) -> P[(m - 1) & 1] -> ... -> P[0] = d_order, so that the
//              last of the m kept passes writes the caller's array whatever m is. m == 0: the iota kernel fills d_order.
//   and per pass p, each kernel returning at once when the plan skips p:
//   count      block t counts byte p of tile t (kSortTile consecutive keys) in LDS, counts[v * tiles + t].
//   scan       block v turns counts[v * tiles ..+ tiles) into the first destination of value v in each tile: the keys
//              with a smaller byte (from hist[p]) plus the keys of value v in earlier tiles, kSortScan tiles per step of a
//              block scan with a carry. This is the exclusive scan in value-major, tile-minor order.
//   scatter    block t, wave w, round r takes the 64 keys from tile t's key (w * kSortRounds + r) * 64 on. Eight ballots
//              (one per bit of the byte) give every lane the mask of the lanes with its byte; its place among them is the
//              number of set bits below it. The wave keeps, per value, the keys of its earlier rounds in LDS (one lane per
//              value adds the round's count, after every lane has read the old one); after the block's barrier the four
//              waves' totals, taken in wave order on top of the scan's number, give every wave its first destination per
//              value. destination = that + earlier rounds + lanes below: tile order, then wave order, then round order,
//              then lane order, which is input order. No atomic takes part, so the permutation is the same in every run,
//              and every pass is stable, which is what makes the least-significant-digit order right.
//
// Plain HIP: no inline assembly; every store is a vector store or, in the histogram and the count, a vector atomic.
// Bounds: a key index is checked against n before every load; a destination is below n because the counts of a pass
// sum to n. n < 2^31 (checked by the entry points), so indices, counts and destinations fit 32 bits.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "drm_device.h"

namespace drm {
namespace {

constexpr int kBlock = kSortBlock;           // 256 lanes, 4 waves
constexpr int kWaves = kBlock / 64;
constexpr int kRounds = kSortRounds;         // keys per lane and tile
constexpr int kTile = kSortTile;             // kBlock * kRounds
constexpr int kScan = kSortScan;             // tiles per step of the scan: one per lane
constexpr int kSortOnes = 8 * 256;           // hist[kSortOnes]: the all-ones keys
constexpr int kHistWords = 8 * 256 + 64;
static_assert(kTile == kBlock * kRounds && kScan == kBlock && kWaves == 4, "the tile shape");

struct PassPlan {
    int32_t keep;     // 0: the pass's kernels return at once
    int32_t key_src;  // 0 = the caller's keys, 1 = K0, 2 = K1
    int32_t key_dst;  // 1 = K0, 2 = K1, 0 = no keys written (the last kept pass)
    int32_t pay_src;  // 0 = the key's own index, 1 = P0 (the caller's order), 2 = P1
    int32_t pay_dst;  // 1 = P0, 2 = P1
};

__device__ __forceinline__ const PassPlan *plan_of(const SortArgs &a, int pass)
{
    return reinterpret_cast<const PassPlan *>(a.plan) + pass;
}
__device__ __forceinline__ const uint64_t *key_buffer(const SortArgs &a, int which)
{
    return which == 0 ? a.keys : which == 1 ? a.k0 : a.k1;
}
__device__ __forceinline__ uint32_t byte_of(uint64_t key, int pass) { return (uint32_t)(key >> (8 * pass)) & 255u; }

// One more key of value v (valid lanes only) in row[256] of LDS counts, for every lane of a wave at once. Real keys
// share their upper bytes: the lanes that agree with the wave's first valid lane add their number once instead of
// queueing at one LDS address; the others add 1 each. Every lane of the wave must call it.
__device__ __forceinline__ void count_value(uint32_t *row, uint32_t v, bool valid)
{
    const unsigned long long live = __ballot(valid);
    if (live == 0)
        return;
    const uint32_t v0 = (uint32_t)__shfl((int)v, __ffsll((long long)live) - 1);
    const unsigned long long same = __ballot(valid && v == v0);
    if (valid && v != v0)
        atomicAdd(&row[v], 1u);
    else if (valid && (int)(threadIdx.x & 63) == __ffsll((long long)same) - 1)
        atomicAdd(&row[v], (uint32_t)__popcll(same));
}

constexpr int kHistKeys = 4; // keys per lane in flight in the histogram's loop

__global__ __launch_bounds__(kBlock) void sort_histogram_kernel(SortArgs a)
{
    __shared__ uint32_t h[8 * 256 + 1]; // the last word: the all-ones keys
    for (int i = threadIdx.x; i < 8 * 256 + 1; i += kBlock)
        h[i] = 0;
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * (kBlock * kHistKeys);
    // every lane of a wave runs the same number of rounds, so that the ballots see the whole wave
    for (int64_t base = (int64_t)blockIdx.x * (kBlock * kHistKeys); base < a.n; base += step) {
        uint64_t key[kHistKeys];
#pragma unroll
        for (int u = 0; u < kHistKeys; ++u) {
            const int64_t i = base + u * kBlock + threadIdx.x;
            key[u] = i < a.n ? a.keys[i] : 0;
        }
#pragma unroll
        for (int u = 0; u < kHistKeys; ++u) {
            const bool valid = base + u * kBlock + threadIdx.x < a.n;
            const unsigned long long ones = __ballot(valid && key[u] == ~0ull);
            if (ones != 0 && (threadIdx.x & 63) == 0)
                atomicAdd(&h[kSortOnes], (uint32_t)__popcll(ones));
#pragma unroll
            for (int p = 0; p < 8; ++p)
                count_value(h + p * 256, byte_of(key[u], p), valid);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 8 * 256 + 1; i += kBlock)
        if (h[i])
            atomicAdd(&a.hist[i], h[i]);
}

__global__ __launch_bounds__(256) void sort_plan_kernel(SortArgs a)
{
    // lane v looks at value v of every byte; the block's votes are the same in every lane
    const uint32_t ones = a.hist[kSortOnes];
    bool drop[8];
    bool have_ones_pass = false;
    for (int p = 0; p < 8; ++p) {
        const uint32_t c = a.hist[p * 256 + threadIdx.x];
        const bool constant = __syncthreads_or((int64_t)c == a.n) != 0;
        const int values = __syncthreads_count(c != 0);
        // byte p only tells the all-ones keys from the rest
        const bool ones_only = ones > 0 && values == 2 && a.hist[p * 256 + 255] == ones;
        drop[p] = constant || (ones_only && have_ones_pass);
        have_ones_pass = have_ones_pass || (ones_only && !constant);
    }
    if (threadIdx.x != 0)
        return;
    PassPlan *plan = reinterpret_cast<PassPlan *>(a.plan);
    int m = 0;
    for (int p = 0; p < 8; ++p)
        m += !drop[p];
    int j = 0;
    for (int p = 0; p < 8; ++p) {
        PassPlan q{};
        if (!drop[p]) {
            q.keep = 1;
            q.key_src = j == 0 ? 0 : 1 + ((j - 1) & 1);
            q.key_dst = j == m - 1 ? 0 : 1 + (j & 1);
            q.pay_src = j == 0 ? 0 : 1 + ((m - j) & 1);
            q.pay_dst = 1 + ((m - 1 - j) & 1);
            ++j;
        }
        plan[p] = q;
    }
    PassPlan none{};
    none.keep = m == 0; // the ninth entry: the iota kernel's
    plan[8] = none;
}

// all keys equal in every byte: the order is the identity
__global__ __launch_bounds__(kBlock) void sort_iota_kernel(SortArgs a)
{
    if (!plan_of(a, 8)->keep)
        return;
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += step)
        a.p0[i] = (uint32_t)i;
}

__global__ __launch_bounds__(kBlock) void sort_count_kernel(SortArgs a, int pass)
{
    const PassPlan pl = *plan_of(a, pass);
    if (!pl.keep)
        return;
    __shared__ uint32_t c[256];
    c[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t *src = key_buffer(a, pl.key_src);
    const int64_t base = (int64_t)blockIdx.x * kTile;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) { // a count: the order of the additions does not matter
        const int64_t i = base + r * kBlock + threadIdx.x;
        const bool valid = i < a.n;
        count_value(c, valid ? byte_of(src[i], pass) : 0u, valid);
    }
    __syncthreads();
    a.counts[(size_t)threadIdx.x * a.tiles + blockIdx.x] = c[threadIdx.x];
}

// the inclusive scan of x over the block's 256 lanes; `total` gets the block's sum
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t x, uint32_t *wave_sum, uint32_t &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, d);
        if (lane >= d)
            x += y;
    }
    __syncthreads(); // wave_sum may still be read by the step before
    if (lane == 63)
        wave_sum[w] = x;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        before += i < w ? wave_sum[i] : 0;
        total += wave_sum[i];
    }
    return x + before;
}

__global__ __launch_bounds__(kBlock) void sort_scan_kernel(SortArgs a, int pass)
{
    if (!plan_of(a, pass)->keep)
        return;
    __shared__ uint32_t wave_sum[kWaves];
    const uint32_t v = blockIdx.x; // this block's byte value
    // the keys whose byte is below v
    const uint32_t mine = threadIdx.x < v ? a.hist[pass * 256 + threadIdx.x] : 0;
    uint32_t carry = 0;
    (void)block_inclusive_scan(mine, wave_sum, carry);
    uint32_t *row = a.counts + (size_t)v * a.tiles;
    for (int64_t t0 = 0; t0 < a.tiles; t0 += kScan) {
        const int64_t t = t0 + threadIdx.x;
        const uint32_t x = t < a.tiles ? row[t] : 0;
        uint32_t total = 0;
        const uint32_t incl = block_inclusive_scan(x, wave_sum, total);
        if (t < a.tiles)
            row[t] = carry + incl - x;
        carry += total;
    }
}

__global__ __launch_bounds__(kBlock) void sort_scatter_kernel(SortArgs a, int pass)
{
    const PassPlan pl = *plan_of(a, pass);
    if (!pl.keep)
        return;
    // [w][v]: first the keys of value v in wave w's rounds so far, then wave w's first destination for value v
    __shared__ uint32_t place[kWaves * 256];
    for (int i = threadIdx.x; i < kWaves * 256; i += kBlock)
        place[i] = 0;
    __syncthreads();
    const uint64_t *src = key_buffer(a, pl.key_src);
    const uint32_t *pay = pl.pay_src == 1 ? a.p0 : a.p1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t *mine = place + w * 256;
    const int64_t base = (int64_t)blockIdx.x * kTile + (int64_t)w * (kRounds * 64);

    uint64_t key[kRounds];
    uint32_t load[kRounds], rank[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const int64_t i = base + r * 64 + lane;
        const bool valid = i < a.n;
        key[r] = valid ? src[i] : 0;
        load[r] = !valid ? 0 : pl.pay_src == 0 ? (uint32_t)i : pay[i];
    }
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        const bool valid = base + r * 64 + lane < a.n;
        const uint32_t v = byte_of(key[r], pass);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (v >> b) & 1u;
            const unsigned long long set = __ballot(bit);
            peers &= bit ? set : ~set;
        }
        // the lanes of one value all read the count of the rounds before, then the lowest of them adds this round's
        const uint32_t before = valid ? mine[v] : 0;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        rank[r] = before + (uint32_t)__popcll(peers & below);
        if (valid && (peers & below) == 0)
            mine[v] = before + (uint32_t)__popcll(peers);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    { // lane v of the block: the waves' totals of value v become their first destinations
        const uint32_t v = threadIdx.x;
        uint32_t next = a.counts[(size_t)v * a.tiles + blockIdx.x];
#pragma unroll
        for (int i = 0; i < kWaves; ++i) {
            const uint32_t c = place[i * 256 + v];
            place[i * 256 + v] = next;
            next += c;
        }
    }
    __syncthreads();
    uint64_t *kdst = pl.key_dst == 1 ? a.k0 : a.k1;
    uint32_t *pdst = pl.pay_dst == 1 ? a.p0 : a.p1;
#pragma unroll
    for (int r = 0; r < kRounds; ++r) {
        if (base + r * 64 + lane >= a.n)
            continue;
        const uint32_t to = mine[byte_of(key[r], pass)] + rank[r];
        if (pl.key_dst != 0)
            kdst[to] = key[r];
        pdst[to] = load[r];
    }
}

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

} // namespace

int64_t sort_tiles(int64_t n) { return (n + kTile - 1) / kTile; }

size_t sort_workspace_bytes(int64_t n)
{
    const size_t tiles = (size_t)sort_tiles(n);
    return align256(sizeof(uint32_t) * kHistWords) + align256(sizeof(PassPlan) * 9) + align256(sizeof(uint32_t) * 256 * tiles) +
           2 * align256(sizeof(uint64_t) * (size_t)n) + align256(sizeof(uint32_t) * (size_t)n);
}

void launch_sort_order(const uint64_t *d_keys, int64_t n, uint32_t *d_order, void *d_work, hipStream_t stream)
{
    if (n <= 0)
        return;
    SortArgs a{};
    a.keys = d_keys;
    a.n = n;
    a.tiles = sort_tiles(n);
    char *w = static_cast<char *>(d_work);
    a.hist = reinterpret_cast<uint32_t *>(w);
    w += align256(sizeof(uint32_t) * kHistWords);
    a.plan = reinterpret_cast<int32_t *>(w);
    w += align256(sizeof(PassPlan) * 9);
    a.counts = reinterpret_cast<uint32_t *>(w);
    w += align256(sizeof(uint32_t) * 256 * (size_t)a.tiles);
    a.k0 = reinterpret_cast<uint64_t *>(w);
    w += align256(sizeof(uint64_t) * (size_t)n);
    a.k1 = reinterpret_cast<uint64_t *>(w);
    w += align256(sizeof(uint64_t) * (size_t)n);
    a.p0 = d_order;
    a.p1 = reinterpret_cast<uint32_t *>(w);

    int dev = 0, cus = 0;
    DRM_HIP_CHECK(hipGetDevice(&dev));
    DRM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    const int64_t lanes_blocks = (n + kBlock - 1) / kBlock;
    const int stride_grid = (int)std::min<int64_t>(lanes_blocks, (int64_t)std::max(cus, 1) * 8);
    // the histogram: four keys a lane and step, at most 4 blocks a CU, each of which ends with up to 2,049 global adds
    const int hist_grid = (int)std::min<int64_t>((lanes_blocks + kHistKeys - 1) / kHistKeys, (int64_t)std::max(cus, 1) * 4);
    DRM_HIP_CHECK(hipMemsetAsync(a.hist, 0, sizeof(uint32_t) * kHistWords, stream));
    hipLaunchKernelGGL(sort_histogram_kernel, dim3(hist_grid), dim3(kBlock), 0, stream, a);
    hipLaunchKernelGGL(sort_plan_kernel, dim3(1), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(sort_iota_kernel, dim3(stride_grid), dim3(kBlock), 0, stream, a);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(sort_count_kernel, dim3((unsigned)a.tiles), dim3(kBlock), 0, stream, a, pass);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(256), dim3(kBlock), 0, stream, a, pass);
        hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)a.tiles), dim3(kBlock), 0, stream, a, pass);
    }
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
