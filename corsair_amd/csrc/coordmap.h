// What coordmap.hip (coordinate maps) and kernelmap.hip (kernel maps) share: the probe of a coordinate map's table, and one
// host function of each unit that the other calls.
#pragma once
#include "common.h"

namespace cs {

// row of `key` in an open-addressing table (linear probing, empty = kEmptyKey), or -1
__device__ __forceinline__ int32_t hash_lookup(const uint64_t* __restrict__ keys,
                                               const int32_t* __restrict__ vals, uint64_t mask,
                                               uint64_t key) {
  uint64_t slot = hash64(key) & mask;
  while (true) {
    uint64_t k = keys[slot];
    if (k == key) return vals[slot];
    if (k == kEmptyKey) return -1;
    slot = (slot + 1) & mask;
  }
}

// coordmap.hip: per-sample segment tables of the maps that do not have them yet (cached on the map, see seg_state)
int ensure_segments_many(cs_coordmap* const* maps, int n, hipStream_t s);
// kernelmap.hip: the one int32 exclusive scan of the two units (n < 2^31)
int exclusive_scan_i32(const int32_t* d_in, int32_t* d_out, int64_t n, hipStream_t s);

}  // namespace cs
