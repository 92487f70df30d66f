// tools/microbench/hipcub_sort.hip -- hipcub::DeviceRadixSort::SortPairs behind a C ABI, the yardstick of
// tools/scripts/sort_bench.py. Not part of libdrm_hip.so: the project's sort is csrc/sort_order.hip.
//   hipcc -O3 --offload-arch=gfx950 -shared -fPIC tools/microbench/hipcub_sort.hip -o tools/microbench/libhipcub_sort.so
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>

extern "C" int hipcub_sort_pairs_bytes(int64_t n, size_t *bytes)
{
    *bytes = 0;
    return (int)hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                   (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0, 64, nullptr);
}

// keys_in / values_in [n] are left unchanged; all 64 bits take part
extern "C" int hipcub_sort_pairs(void *tmp, size_t bytes, const uint64_t *keys_in, uint64_t *keys_out,
                                 const uint32_t *values_in, uint32_t *values_out, int64_t n, void *stream)
{
    return (int)hipcub::DeviceRadixSort::SortPairs(tmp, bytes, keys_in, keys_out, values_in, values_out, (int)n, 0, 64,
                                                   (hipStream_t)stream);
}
