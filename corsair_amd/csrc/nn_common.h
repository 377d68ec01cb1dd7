// What knn.hip, topk.hip and chamfer.hip share: the matrix-core operand types, the f16 hi / lo cut, the host
// helpers of their drivers, and the two kernels that two of them launch (each defined once, in one unit, and
// reached from the other through an ordinary host function).
#pragma once
#include <stdlib.h>

#include <atomic>
#include <vector>

#include "common.h"

namespace cs {

using f64x4 = __attribute__((ext_vector_type(4))) double;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ void knf_split(float v, _Float16* hi, _Float16* lo) {
  const _Float16 h = (_Float16)v;
  *hi = h;
  *lo = (_Float16)(v - (float)h);
}

template <typename T>
static int upload(PoolBuf<T>& buf, const std::vector<T>& host, hipStream_t s) {
  if (!buf.alloc(host.size())) return CS_ERR_HIP;
  if (!host.empty())
    CS_HIP_CHECK(hipMemcpyAsync(buf.p, host.data(), host.size() * sizeof(T),
                                hipMemcpyHostToDevice, s));
  // pageable source: the runtime has staged the bytes when the call returns
  return CS_OK;
}

// Environment switches are read once per call, in each family's read_options(): tests flip them between the
// calls of one process, so none is cached.  INTEGRATION.md lists them.
inline bool env_first_is(const char* name, char c) {
  const char* e = getenv(name);
  return e && e[0] == c;
}

// out[i] = sum_c X[i, c]^2, one f64 fma chain per row (k_row_norms, topk.hip).  Launch only: the caller's
// CS_LAUNCH_CHECK covers it.
void row_norms(const float* d_x, int64_t n, int d, double* d_out, hipStream_t s);

// *host_out = number of non-zero entries of flag[0, n) (k_count_flags, knn.hip).  Waits for the stream: only the
// statistics switches call it.  `who` prefixes the error text.
int count_flagged(const int32_t* d_flag, int64_t n, unsigned long long* host_out, hipStream_t s, const char* who);

// the body of every cs_*_stats getter: {items answered by the fast path, of those recomputed by its fallback}
inline void read_stats(std::atomic<unsigned long long> (&stats)[2], uint64_t out[2], int reset) {
  for (int i = 0; i < 2; ++i) {
    if (out) out[i] = stats[i].load();
    if (reset) stats[i].store(0);
  }
}

}  // namespace cs
