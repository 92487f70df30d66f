// deepreadmapper_amd/csrc/bgzf.hip -- BGZF compression on the device, for gfx950 (drm_bgzf_compress, include/drm_hip.h;
// DESIGN.md sec. 4.20).
//
// One workgroup of 1024 lanes turns one block of at most 65,280 input bytes into one complete gzip member (header with
// the BC subfield, one raw DEFLATE block with BFINAL = 1, CRC-32, ISIZE) in the block's 65,536-byte slot. A one-block
// scan then turns the members' sizes into offsets and a copy packs the members back to back.
//
//   load     the block's bytes into LDS (zero-padded), where every later step reads them.
//   crc      lane i takes bytes [64 i, 64 i + 64): its own CRC-32, moved past the bytes behind it by a multiplication
//            with x^(8 m) mod P (built from the precomputed x^(8 * 2^k)), then an XOR over the block -- the CRC is
//            linear, crc(A || B) = shift(crc(A), |B|) ^ crc(B).
//   count    the LZ77 parse, a tile of 1024 positions at a time, one position per lane:
//     candidates  the hash of the four bytes at p gives (a) head[h], the last position of an earlier tile with that
//                 hash -- every lane reads it before the barrier behind which the tile's own positions go in by an LDS
//                 atomicMax -- and (b) first[h'], the first position of this tile with that hash, by an LDS atomicMin
//                 into a table that is cleared per tile. Maximum and minimum do not depend on the order of their
//                 updates, so the candidates, and with them the member, are a function of the block's bytes alone.
//     match       both candidates are compared with p word by word in LDS, up to min(258, n - p) bytes: a match never
//                 leaves the block, and a candidate farther back than 32,768 is dropped. The longer one wins, the
//                 nearer one on a tie. Minimum match 4.
//     parse       greedy: from the tile's entry position, a match of >= 4 jumps its length, anything else one byte.
//                 next[p] is known for every p at once, so the positions the walk visits are found by pointer
//                 jumping: 11 rounds of mark[jump[p]] |= mark[p]; jump[p] = jump[jump[p]] cover the 1024 steps a tile
//                 can hold. A jump past the tile's end lands on one of 258 sink entries; the marked sink is the next
//                 tile's entry.
//     tokens      a block scan of the marks compacts the visited positions' tokens (literal, or length and distance)
//                 into the workgroup's scratch in global memory, and their fixed-Huffman bit lengths are added up.
//   choose   only the count tells the form: fixed Huffman when its payload is at most n + 5 bytes, else stored. (At nine
//            bits a literal >= 144 the fixed form of a full block of such bytes would not fit the slot.)
//   emit     fixed: the member is assembled in LDS, in the 64 KiB the hash heads no longer need: a block scan of the
//            tokens' bit lengths gives every token its bit offset, and its bits are ORed into two 32-bit words (an OR
//            does not depend on order either). Huffman codes are bit-reversed first, so that they read most significant
//            bit first in a stream that is filled from bit 0. Stored: header, 01 LEN ~LEN, the bytes. Either way the
//            slot is then written word by word.
//
// Plain HIP: no inline assembly; every store is a vector store or a vector / LDS atomic.
// Bounds: LDS input reads stay below word kInWords (the last hashed position is n - 4, the last compared byte n - 1, and
// the unaligned 32-bit read takes one word more); a jump is at most 1023 + 258 = kJump - 1; a token index is below the
// block's length; a fixed member is at most n + 31 <= 65,311 bytes, below the 65,536 of the LDS image and of the slot.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "drm_device.h"

namespace drm {
namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kTile = kThreads;                  // positions per step of the parse, one per lane
constexpr int kHeadBits = 14, kFirstBits = 11;   // hash heads of the block; first positions of the tile
constexpr int kMinMatch = 4, kMaxMatch = 258, kMaxDist = 32768;
constexpr int kInWords = kBgzfBlock / 4 + 2;     // the block, zero-padded by 8 bytes
constexpr int kImageWords = 1 << kHeadBits;      // 64 KiB: the hash heads, then the member's image
constexpr int kJump = kTile + kMaxMatch;         // tile positions, then the sinks 1024 .. 1281
constexpr int kRounds = 11;                      // 2^11 > 1024 steps
constexpr int kHeader = 18, kTrailer = 8;
constexpr uint32_t kPoly = 0xEDB88320u, kHashMul = 2654435761u;
static_assert(kBgzfBlock % 4 == 0 && kBgzfBlock <= 64 * kThreads, "64 bytes of CRC a lane cover a block");
static_assert(kBgzfBlock + 5 + kHeader + kTrailer <= 4 * kImageWords && 4 * kImageWords <= kBgzfSlot, "a member fits");

struct Lds {
    uint32_t in[kInWords];
    uint32_t image[kImageWords];
    uint32_t first[1 << kFirstBits];
    uint16_t jump[kJump + 2];
    uint8_t mark[kJump + 2];
    uint32_t wave_sum[kWaves];
    uint32_t entry, crc;
};
static_assert(sizeof(Lds) <= 160 * 1024, "the LDS of one CU");

// a(x) * b(x) mod P over GF(2), bit 31 the coefficient of x^0 (the reflected form of CRC-32)
__host__ __device__ constexpr uint32_t gf_mult(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (kPoly & (0u - (b & 1u)));
    }
    return p;
}

// x^(8 * 2^k) mod P, k = 0 .. 16
struct ShiftTable {
    uint32_t v[17];
};
constexpr ShiftTable make_shift_table()
{
    ShiftTable t{};
    uint32_t p = 0x00800000u; // x^8
    for (int k = 0; k < 17; ++k) {
        t.v[k] = p;
        p = gf_mult(p, p);
    }
    return t;
}
__constant__ ShiftTable kShift = make_shift_table();

// the finished CRC-32 of a string, as the CRC of that string followed by `bytes` more bytes would hold it (before those
// bytes' own contribution)
__device__ __forceinline__ uint32_t crc_shift(uint32_t crc, uint32_t bytes)
{
    uint32_t op = 0x80000000u; // x^0
    for (int k = 0; k < 17; ++k)
        if ((bytes >> k) & 1u)
            op = gf_mult(kShift.v[k], op);
    return gf_mult(op, crc);
}

__device__ __forceinline__ uint32_t crc_bits(uint32_t crc, int bits)
{
    for (int i = 0; i < bits; ++i)
        crc = (crc >> 1) ^ (kPoly & (0u - (crc & 1u)));
    return crc;
}

// four bytes from byte `pos` of the LDS words, little-endian, at any alignment
__device__ __forceinline__ uint32_t load32(const uint32_t *words, int pos)
{
    const uint64_t w = ((uint64_t)words[(pos >> 2) + 1] << 32) | words[pos >> 2];
    return (uint32_t)(w >> (8 * (pos & 3)));
}
__device__ __forceinline__ uint32_t load8(const uint32_t *words, int pos)
{
    return (words[pos >> 2] >> (8 * (pos & 3))) & 255u;
}

// the bytes that agree from c and from p on, at most maxlen (c < p; the two ranges may overlap, as in LZ77)
__device__ __forceinline__ int match_length(const uint32_t *words, int c, int p, int maxlen)
{
    int i = 0;
    while (i < maxlen) {
        const uint32_t x = load32(words, c + i) ^ load32(words, p + i);
        if (x != 0) {
            i += (__ffs((int)x) - 1) >> 3;
            break;
        }
        i += 4;
    }
    return min(i, maxlen);
}

// the exclusive scan of x over the block's 1024 lanes; `total` gets the block's sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t x, uint32_t *wave_sum, uint32_t &total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= d)
            incl += y;
    }
    __syncthreads(); // wave_sum may still be read by the scan before
    if (lane == 63)
        wave_sum[w] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        const uint32_t s = wave_sum[i];
        before += i < w ? s : 0;
        total += s;
    }
    return before + incl - x;
}

// `bits` low bits of a Huffman code, first bit of the code in bit 0
__device__ __forceinline__ uint32_t reversed(uint32_t code, int bits) { return __brev(code) >> (32 - bits); }

// the fixed-Huffman bits of a literal or of the end-of-block / length symbol `sym` (RFC 1951 sec. 3.2.6)
__device__ __forceinline__ void litlen_code(uint32_t sym, uint32_t &v, int &nb)
{
    if (sym < 144u) {
        nb = 8;
        v = reversed(0x30u + sym, 8);
    } else if (sym < 256u) {
        nb = 9;
        v = reversed(0x190u + (sym - 144u), 9);
    } else if (sym < 280u) {
        nb = 7;
        v = reversed(sym - 256u, 7);
    } else {
        nb = 8;
        v = reversed(0xC0u + (sym - 280u), 8);
    }
}

// the bits of one match, filled from bit 0: the length's code and extra bits, the distance's 5-bit code and extra bits;
// at most 8 + 5 + 5 + 13 = 31
__device__ __forceinline__ void match_code(int len, int dist, uint32_t &v, int &nb)
{
    const uint32_t l = (uint32_t)(len - 3);
    uint32_t sym, extra = 0;
    int e = 0;
    if (len == kMaxMatch) {
        sym = 285u;
    } else if (l < 8u) {
        sym = 257u + l;
    } else {
        e = (31 - __clz((int)l)) - 2;
        sym = 261u + 4u * (uint32_t)e + ((l >> e) & 3u);
        extra = l & ((1u << e) - 1u);
    }
    litlen_code(sym, v, nb);
    v |= extra << nb;
    nb += e;
    const uint32_t d = (uint32_t)(dist - 1);
    uint32_t dsym, dextra = 0;
    int de = 0;
    if (d < 4u) {
        dsym = d;
    } else {
        const int k = 31 - __clz((int)d);
        de = k - 1;
        dsym = 2u * (uint32_t)k + ((d >> (k - 1)) & 1u);
        dextra = d & ((1u << de) - 1u);
    }
    v |= reversed(dsym, 5) << nb;
    nb += 5;
    v |= dextra << nb;
    nb += de;
}

// a token word: a literal is its byte; a match has bit 31, length - 3 in bits 16 .. 23 and distance - 1 in bits 0 .. 14
__device__ __forceinline__ void token_code(uint32_t word, uint32_t &v, int &nb)
{
    if (word >> 31)
        match_code((int)((word >> 16) & 255u) + 3, (int)(word & 32767u) + 1, v, nb);
    else
        litlen_code(word & 255u, v, nb);
}

// ORs the low `nb` <= 32 bits of v into the image from bit `at` on
__device__ __forceinline__ void or_bits(uint32_t *image, uint32_t at, uint32_t v)
{
    const uint32_t w = at >> 5, sh = at & 31u;
    const uint64_t x = (uint64_t)v << sh;
    if ((uint32_t)x != 0)
        atomicOr(&image[w], (uint32_t)x);
    if ((uint32_t)(x >> 32) != 0)
        atomicOr(&image[w + 1], (uint32_t)(x >> 32));
}

// byte j of a stored member of n bytes with the given CRC
__device__ __forceinline__ uint32_t stored_byte(const uint32_t *in, int n, uint32_t crc, int j)
{
    const uint32_t bsize1 = (uint32_t)(n + 5 + kHeader + kTrailer - 1);
    const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    if (j < 16)
        return head[j];
    if (j < 18)
        return (bsize1 >> (8 * (j - 16))) & 255u;
    if (j == 18)
        return 1u; // BFINAL = 1, BTYPE = 00
    if (j < 21)
        return ((uint32_t)n >> (8 * (j - 19))) & 255u;
    if (j < 23)
        return (~(uint32_t)n >> (8 * (j - 21))) & 255u;
    if (j < 23 + n)
        return load8(in, j - 23);
    if (j < 27 + n)
        return (crc >> (8 * (j - 23 - n))) & 255u;
    return ((uint32_t)n >> (8 * (j - 27 - n))) & 255u;
}

__global__ __launch_bounds__(kThreads) void bgzf_deflate_kernel(BgzfArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_bytes[];
    Lds &s = *reinterpret_cast<Lds *>(lds_bytes);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t *tokens = a.tokens + (size_t)blockIdx.x * kBgzfBlock;

    for (int64_t b = blockIdx.x; b < a.blocks; b += gridDim.x) {
        const int n = (int)min((int64_t)kBgzfBlock, a.n - b * kBgzfBlock);
        const uint8_t *src = a.data + b * kBgzfBlock;

        // ---------------------------------------------------------------------------------------- load
        const bool aligned = (reinterpret_cast<uintptr_t>(src) & 3u) == 0;
        for (int w = tid; w < kInWords; w += kThreads) {
            const int j = 4 * w;
            uint32_t x = 0;
            if (aligned && j + 4 <= n) {
                x = *reinterpret_cast<const uint32_t *>(src + j);
            } else {
                for (int q = 0; q < 4; ++q)
                    if (j + q < n)
                        x |= (uint32_t)src[j + q] << (8 * q);
            }
            s.in[w] = x;
        }
        for (int i = tid; i < kImageWords; i += kThreads)
            s.image[i] = 0; // the hash heads: 0 = none, else position + 1
        if (tid == 0)
            s.entry = 0;
        __syncthreads();

        // ----------------------------------------------------------------------------------------- crc
        {
            const int from = 64 * tid, mine = max(0, min(64, n - from));
            uint32_t part = 0;
            if (mine > 0) {
                uint32_t c = ~0u;
                int i = 0;
                for (; i + 4 <= mine; i += 4)
                    c = crc_bits(c ^ s.in[(from + i) >> 2], 32);
                for (; i < mine; ++i)
                    c = crc_bits(c ^ load8(s.in, from + i), 8);
                part = crc_shift(~c, (uint32_t)(n - from - mine));
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1)
                part ^= (uint32_t)__shfl_xor((int)part, d);
            if (lane == 0)
                s.wave_sum[wave] = part;
            __syncthreads();
            if (tid == 0) {
                uint32_t c = 0;
                for (int i = 0; i < kWaves; ++i)
                    c ^= s.wave_sum[i];
                s.crc = c;
            }
            // the scans below start with a barrier, so wave_sum is free again by then
        }

        // --------------------------------------------------------------------------------------- count
        uint32_t ntok = 0, my_bits = 0;
        const int tiles = (n + kTile - 1) / kTile;
        for (int t = 0; t < tiles; ++t) {
            const int p = t * kTile + tid;
            const bool live = p < n, hashed = p + kMinMatch <= n;
            s.first[tid] = ~0u;
            s.first[tid + kThreads] = ~0u;
            s.mark[tid] = 0;
            if (tid < kJump - kTile) {
                s.mark[kTile + tid] = 0;
                s.jump[kTile + tid] = (uint16_t)(kTile + tid); // a sink stays where it is
            }
            uint32_t h = 0, h2 = 0, head = 0;
            if (hashed) {
                const uint32_t x = load32(s.in, p) * kHashMul;
                h = x >> (32 - kHeadBits);
                h2 = x >> (32 - kFirstBits);
                head = s.image[h];
            }
            __syncthreads(); // every head is read, every first[] cleared
            if (hashed) {
                atomicMax(&s.image[h], (uint32_t)p + 1u);
                atomicMin(&s.first[h2], (uint32_t)p);
            }
            __syncthreads();
            int len = 0, dist = 0;
            if (hashed) {
                const int maxlen = min(kMaxMatch, n - p);
                const uint32_t c2 = s.first[h2];
                if (c2 < (uint32_t)p) {
                    const int l = match_length(s.in, (int)c2, p, maxlen);
                    if (l >= kMinMatch) {
                        len = l;
                        dist = p - (int)c2;
                    }
                }
                if (head != 0 && p - (int)(head - 1u) <= kMaxDist) {
                    const int l = match_length(s.in, (int)(head - 1u), p, maxlen);
                    if (l >= kMinMatch && l > len) {
                        len = l;
                        dist = p - (int)(head - 1u);
                    }
                }
            }
            // a position past the block's end stays where it is, like a sink
            s.jump[tid] = (uint16_t)(live ? tid + (len >= kMinMatch ? len : 1) : tid);
            __syncthreads();
            if (tid == 0)
                s.mark[s.entry] = 1;
            __syncthreads();
            for (int r = 0; r < kRounds; ++r) {
                // a mark set by another lane in this round and seen here only marks a later position of the same walk
                const uint32_t j = s.jump[tid];
                if (s.mark[tid])
                    s.mark[j] = 1;
                const uint16_t j2 = s.jump[j];
                __syncthreads();
                s.jump[tid] = j2;
                __syncthreads();
            }
            const bool token = live && s.mark[tid] != 0;
            if (tid < kJump - kTile && s.mark[kTile + tid])
                s.entry = (uint32_t)tid; // the one sink the walk reached
            uint32_t word = 0;
            if (token) {
                uint32_t v;
                int nb;
                word = len >= kMinMatch ? (1u << 31) | ((uint32_t)(len - 3) << 16) | (uint32_t)(dist - 1) : load8(s.in, p);
                token_code(word, v, nb);
                my_bits += (uint32_t)nb;
            }
            uint32_t total = 0;
            const uint32_t rank = block_exclusive_scan(token ? 1u : 0u, s.wave_sum, total);
            if (token)
                tokens[ntok + rank] = word;
            ntok += total;
        }

        // -------------------------------------------------------------------------------------- choose
        uint32_t token_bits = 0;
        (void)block_exclusive_scan(my_bits, s.wave_sum, token_bits);
        const uint32_t payload = (3u + token_bits + 7u + 7u) / 8u; // header bits, tokens, end of block, padded
        const bool fixed = payload <= (uint32_t)n + 5u;
        const uint32_t member = kHeader + (fixed ? payload : (uint32_t)n + 5u) + kTrailer;
        uint32_t *slot = reinterpret_cast<uint32_t *>(a.slots + (size_t)b * kBgzfSlot);
        const uint32_t crc = s.crc; // written before the count's barriers

        // ---------------------------------------------------------------------------------------- emit
        if (fixed) {
            for (int i = tid; i < kImageWords; i += kThreads)
                s.image[i] = 0;
            __syncthreads(); // also: the tokens written above are visible to the whole workgroup
            if (tid == 0) {
                s.image[0] = 0x04088b1fu;
                s.image[2] = 0x0006ff00u;
                s.image[3] = 0x00024342u;
                atomicOr(&s.image[4], (member - 1u) | (3u << 16)); // BSIZE - 1; BFINAL = 1, BTYPE = 01
                or_bits(s.image, 8u * (kHeader + payload), crc);
                or_bits(s.image, 8u * (kHeader + payload) + 32u, (uint32_t)n);
            }
            uint32_t at = 8u * kHeader + 3u;
            for (uint32_t i0 = 0; i0 < ntok; i0 += kThreads) {
                uint32_t v = 0;
                int nb = 0;
                if (i0 + tid < ntok)
                    token_code(tokens[i0 + tid], v, nb);
                uint32_t total = 0;
                const uint32_t off = block_exclusive_scan((uint32_t)nb, s.wave_sum, total);
                if (nb != 0)
                    or_bits(s.image, at + off, v);
                at += total;
            }
            __syncthreads();
            for (uint32_t w = tid; w < (member + 3u) / 4u; w += kThreads)
                slot[w] = s.image[w];
        } else {
            for (uint32_t w = tid; w < (member + 3u) / 4u; w += kThreads) {
                uint32_t x = 0;
                for (int q = 0; q < 4; ++q)
                    if (4u * w + q < member)
                        x |= stored_byte(s.in, n, crc, (int)(4u * w) + q) << (8 * q);
                slot[w] = x;
            }
        }
        if (tid == 0)
            a.sizes[b] = member;
        __syncthreads(); // the next block reuses all of it
    }
}

// offsets[b] = the bytes of the members before b; offsets[blocks] = the stream's length. One block.
__global__ __launch_bounds__(kThreads) void bgzf_scan_kernel(BgzfArgs a)
{
    __shared__ uint32_t wave_sum[kWaves];
    uint64_t carry = 0;
    for (int64_t b0 = 0; b0 < a.blocks; b0 += kThreads) {
        const int64_t b = b0 + threadIdx.x;
        const uint32_t x = b < a.blocks ? a.sizes[b] : 0;
        uint32_t total = 0; // at most 1024 members of less than 2^16 bytes
        const uint32_t before = block_exclusive_scan(x, wave_sum, total);
        if (b < a.blocks)
            a.offsets[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0)
        a.offsets[a.blocks] = carry;
}

// member b's bytes to their place in the packed stream. The slot is 4-byte aligned, the destination is wherever the
// members before end: up to three bytes bring the destination to a word, then every lane writes whole words, each put
// together from the two slot words it straddles (the second may lie behind the member, inside the slot; at a shift of
// 0 none of its bits are used), then the last bytes.
__global__ __launch_bounds__(256) void bgzf_pack_kernel(BgzfArgs a)
{
    const int64_t b = blockIdx.x;
    const uint8_t *src = a.slots + (size_t)b * kBgzfSlot;
    const uint32_t *src_words = reinterpret_cast<const uint32_t *>(src);
    uint8_t *dst = a.out + a.offsets[b];
    const uint32_t size = a.sizes[b];
    const uint32_t head = min(size, (uint32_t)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
    const uint32_t words = (size - head) / 4u;
    if (threadIdx.x < head)
        dst[threadIdx.x] = src[threadIdx.x];
    uint32_t *dst_words = reinterpret_cast<uint32_t *>(dst + head);
    for (uint32_t i = threadIdx.x; i < words; i += 256) {
        const uint32_t w = (head + 4u * i) >> 2; // at most (65,311 - 4) / 4, so w + 1 is inside the slot
        const uint64_t both = ((uint64_t)src_words[w + 1] << 32) | src_words[w];
        dst_words[i] = (uint32_t)(both >> (8u * head));
    }
    const uint32_t tail = head + 4u * words + threadIdx.x;
    if (tail < size)
        dst[tail] = src[tail];
}

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

BgzfArgs carve(const uint8_t *d_data, int64_t n, uint8_t *d_out, uint32_t *d_sizes, void *d_work)
{
    BgzfArgs a{};
    a.data = d_data;
    a.n = n;
    a.blocks = bgzf_blocks(n);
    a.out = d_out;
    a.sizes = d_sizes;
    char *w = static_cast<char *>(d_work);
    a.offsets = reinterpret_cast<uint64_t *>(w);
    w += align256(sizeof(uint64_t) * (size_t)(a.blocks + 1));
    a.slots = reinterpret_cast<uint8_t *>(w);
    w += (size_t)a.blocks * kBgzfSlot;
    a.tokens = reinterpret_cast<uint32_t *>(w);
    return a;
}

} // namespace

int64_t bgzf_blocks(int64_t n) { return (n + kBgzfBlock - 1) / kBgzfBlock; }

size_t bgzf_workspace_bytes(int64_t n)
{
    const size_t blocks = (size_t)bgzf_blocks(n);
    return align256(sizeof(uint64_t) * (blocks + 1)) + blocks * kBgzfSlot +
           align256(sizeof(uint32_t) * kBgzfBlock * std::min<size_t>(blocks, kBgzfGrid));
}

const uint64_t *bgzf_total(const void *d_work, int64_t n)
{
    return reinterpret_cast<const uint64_t *>(d_work) + bgzf_blocks(n);
}

void launch_bgzf(const uint8_t *d_data, int64_t n, uint8_t *d_out, uint32_t *d_sizes, void *d_work, hipStream_t stream)
{
    if (n <= 0)
        return;
    const BgzfArgs a = carve(d_data, n, d_out, d_sizes, d_work);
    // more than the 64 KiB a kernel gets without asking: one workgroup a CU
    // asked once per device
    static std::atomic<uint64_t> asked{0};
    int dev = 0;
    DRM_HIP_CHECK(hipGetDevice(&dev));
    const uint64_t bit = dev < 64 ? 1ull << dev : 0;
    if (!(asked.load() & bit)) {
        DRM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(bgzf_deflate_kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Lds)));
        asked.fetch_or(bit);
    }
    const unsigned grid = (unsigned)std::min<int64_t>(a.blocks, kBgzfGrid);
    hipLaunchKernelGGL(bgzf_deflate_kernel, dim3(grid), dim3(kThreads), sizeof(Lds), stream, a);
    hipLaunchKernelGGL(bgzf_scan_kernel, dim3(1), dim3(kThreads), 0, stream, a);
    hipLaunchKernelGGL(bgzf_pack_kernel, dim3((unsigned)a.blocks), dim3(256), 0, stream, a);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
