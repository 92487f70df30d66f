// deepreadmapper_amd/csrc/dup_set.hip -- the first-seen duplicate set, for gfx950.
//
// The duplicate marker of the SAM tail (include/drm_hip.h, drm_dupset_mark): an open-addressing hash set that lives in
// HBM across the blocks of a run and answers, for every item of a call, the smallest item index seen so far with the
// item's key (the unordered pair of its two end words).
//
// Data: keys[max_items], 16 bytes each (lo, hi), written once per item and never changed;
// slots[2^s] u64, 2^s the smallest power of two >= 2 * max_items, a slot holding 0 when empty, else item index + 1.
// The key of a slot's occupant is keys[content - 1]: the table stores no key bytes of its own.
//
// Three launches per call, one lane per item, grid-stride loops:
//   keys    the call's end words, ordered (lo = min, hi = max), into keys[first_item ..).
//   insert  linear probing from dup_hash(lo, hi) & (slots - 1): read the slot; empty: compare-and-swap 0 -> item + 1 and
//           stop on success, else go on with the value the swap returned as the slot's content; content whose key equals
//           the item's: atomic min of item + 1 into the slot, stop; any other content: the next slot, wrapping at the end.
//   resolve the same walk to the slot whose occupant has the item's key: first = content - 1.
//
// Memory rules. Inside the insert kernel a slot is read while other workgroups, on other XCDs with L2s of their own,
// run atomics on it: those reads are agent-scope atomic loads, never plain loads, and the swap and the min are
// agent-scope atomics (vector memory instructions, performed at the device's coherence point). keys[] is only ever read
// for an item whose key an earlier kernel wrote -- the keys kernel of this call or of an earlier one -- so plain loads
// are right there, and the resolve kernel is separated from the inserts by the kernel boundary, so its slot reads are
// plain loads too. A min that replaces an occupant only ever swaps in an item with the same key, so what a concurrent
// prober concludes from comparing keys[content - 1] with its own key does not depend on which of the two it read; and a
// slot, once occupied, is never emptied, so every item of one key walks the same slots to the same one. No deletions
// and a load of at most 1/2 keep an empty slot on every walk; the loops are bounded by the table size all the same.
// Plain HIP: no inline assembly, and every store is a vector store or a vector atomic.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "drm_device.h"

namespace drm {
namespace {

constexpr int kDupBlock = 256;

__device__ __forceinline__ uint64_t load_slot_agent(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kDupBlock) void dup_keys_kernel(DupArgs a)
{
    const int64_t step = (int64_t)gridDim.x * kDupBlock;
    for (int64_t i = (int64_t)blockIdx.x * kDupBlock + threadIdx.x; i < a.n; i += step) {
        const uint64_t e1 = a.ends[2 * i], e2 = a.ends[2 * i + 1]; // the caller's array need not be 16-byte aligned
        reinterpret_cast<ulonglong2 *>(a.keys)[a.first_item + i] = make_ulonglong2(e1 < e2 ? e1 : e2, e1 < e2 ? e2 : e1);
    }
}

__global__ __launch_bounds__(kDupBlock) void dup_insert_kernel(DupArgs a)
{
    const ulonglong2 *keys = reinterpret_cast<const ulonglong2 *>(a.keys);
    const uint64_t mask = a.slot_mask;
    const int64_t step = (int64_t)gridDim.x * kDupBlock;
    for (int64_t i = (int64_t)blockIdx.x * kDupBlock + threadIdx.x; i < a.n; i += step) {
        const uint64_t item = (uint64_t)(a.first_item + i);
        const ulonglong2 key = keys[item];
        if (key.y == 0) // no mapped mate: no key
            continue;
        uint64_t s = dup_hash(key.x, key.y) & mask;
        for (uint64_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
            unsigned long long *slot = a.slots + s;
            uint64_t c = load_slot_agent(slot);
            if (c == 0) {
                unsigned long long expected = 0;
                if (__hip_atomic_compare_exchange_strong(slot, &expected, (unsigned long long)(item + 1), __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                    break;
                c = expected; // the occupant that won the slot
            }
            // c - 1 < max_items: a slot only ever receives the index of an item that passed the entry point's range check
            const ulonglong2 other = keys[c - 1];
            if (other.x == key.x && other.y == key.y) {
                // the occupant may since have been replaced, but only by an item of this same key
                __hip_atomic_fetch_min(slot, (unsigned long long)(item + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
}

__global__ __launch_bounds__(kDupBlock) void dup_resolve_kernel(DupArgs a)
{
    const ulonglong2 *keys = reinterpret_cast<const ulonglong2 *>(a.keys);
    const uint64_t mask = a.slot_mask;
    const int64_t step = (int64_t)gridDim.x * kDupBlock;
    for (int64_t i = (int64_t)blockIdx.x * kDupBlock + threadIdx.x; i < a.n; i += step) {
        const ulonglong2 key = keys[a.first_item + i];
        int64_t first = -1;
        if (key.y != 0) {
            uint64_t s = dup_hash(key.x, key.y) & mask;
            for (uint64_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
                const uint64_t c = a.slots[s]; // after the insert kernel: a plain load
                if (c == 0) // not reached: the insert kernel placed this key on this walk
                    break;
                const ulonglong2 other = keys[c - 1];
                if (other.x == key.x && other.y == key.y) {
                    first = (int64_t)(c - 1);
                    break;
                }
            }
        }
        a.first[i] = first;
    }
}

} // namespace

void launch_dup_mark(const DupArgs &a, hipStream_t stream)
{
    if (a.n <= 0)
        return;
    int dev = 0, cus = 0;
    DRM_HIP_CHECK(hipGetDevice(&dev));
    DRM_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // one lane per item up to 8 blocks of 4 waves per CU, the rest by the grid-stride loops
    const int grid = (int)std::min<int64_t>((a.n + kDupBlock - 1) / kDupBlock, (int64_t)std::max(cus, 1) * 8);
    hipLaunchKernelGGL(dup_keys_kernel, dim3(grid), dim3(kDupBlock), 0, stream, a);
    hipLaunchKernelGGL(dup_insert_kernel, dim3(grid), dim3(kDupBlock), 0, stream, a);
    hipLaunchKernelGGL(dup_resolve_kernel, dim3(grid), dim3(kDupBlock), 0, stream, a);
    DRM_HIP_CHECK(hipGetLastError());
}

} // namespace drm
