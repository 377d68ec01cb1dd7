// The host side of cs_sc2_batch (sc2.hip) that needs no device: the argument checks and the chunk planner.  Plain C++, no
// HIP header, so that tools/sc2_plan_check.cpp can run both under the host sanitizers (view_plan.h's pattern).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

namespace cs {

constexpr int SC2_MAX_CAP = 32768;                  // slots of one problem: its bit matrix is 128 MiB
constexpr int SC2_MIN_K = 2, SC2_MAX_K = 64;        // k_consensus
constexpr int64_t SC2_CHUNK_BYTES = 256LL << 20;    // matrix bytes per chunk unless CS_SC2_CHUNK_BYTES says otherwise

// The codes of include/corsair_hip.h (CS_OK, CS_ERR_INVALID, CS_ERR_UNSUPPORTED), restated so that this header stands alone.
constexpr int SC2_OK = 0, SC2_INVALID = -1, SC2_UNSUPPORTED = -5;

inline bool sc2_positive_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }   // false for NaN

// u64 words of one matrix row, and the bytes of the matrix, of a problem of `cap` slots: one bit per ordered pair
inline int64_t sc2_words(int64_t cap) { return (cap + 63) / 64; }
inline int64_t sc2_matrix_bytes(int64_t cap) { return 8 * cap * sc2_words(cap); }

// The refusals of cs_sc2_batch in the order of the header; msg (at least 200 bytes) holds the reason of a refusal.
inline int sc2_check_args(const void* d_src, const void* d_tgt, const int64_t* h_off, int n_prob, double compat_dist,
                          double max_corr, int n_seeds, int k_consensus, const void* d_T, const void* d_stat,
                          const void* d_rmse, char* msg, size_t msg_len) {
  const char* who = "cs_sc2_batch";
#define SC2_REFUSE(cond, code, ...)         \
  do {                                      \
    if (!(cond)) {                          \
      snprintf(msg, msg_len, __VA_ARGS__);  \
      return (code);                        \
    }                                       \
  } while (0)
  SC2_REFUSE(h_off, SC2_INVALID, "%s: NULL offset table", who);
  SC2_REFUSE(n_prob >= 0, SC2_INVALID, "%s: negative problem count", who);
  int64_t rows = 0;
  for (int p = 0; p < n_prob; ++p) {
    const int64_t sn = h_off[p + 1] - h_off[p];
    SC2_REFUSE(h_off[p] >= 0 && sn >= 0, SC2_INVALID, "%s: bad pair segment %d", who, p);
    rows += sn;
  }
  SC2_REFUSE(sc2_positive_finite(compat_dist), SC2_INVALID, "%s: compat_dist must be positive and finite", who);
  SC2_REFUSE(sc2_positive_finite(max_corr), SC2_INVALID, "%s: max_corr must be positive and finite", who);
  SC2_REFUSE(n_seeds >= 0, SC2_INVALID, "%s: negative n_seeds", who);
  SC2_REFUSE(k_consensus >= SC2_MIN_K && k_consensus <= SC2_MAX_K, SC2_UNSUPPORTED, "%s: k_consensus outside [%d, %d]", who,
             SC2_MIN_K, SC2_MAX_K);
  for (int p = 0; p < n_prob; ++p)
    SC2_REFUSE(h_off[p + 1] - h_off[p] <= SC2_MAX_CAP, SC2_UNSUPPORTED,
               "%s: problem %d has more than %d slots (its bit matrix would exceed 128 MiB): build the lists with a smaller "
               "k_nn",
               who, p, SC2_MAX_CAP);
  SC2_REFUSE(n_prob == 0 || (d_T && d_stat && d_rmse), SC2_INVALID, "%s: NULL output", who);
  SC2_REFUSE(rows == 0 || (d_src && d_tgt), SC2_INVALID, "%s: NULL d_src or d_tgt", who);
#undef SC2_REFUSE
  return SC2_OK;
}

// matrix bytes per chunk: CS_SC2_CHUNK_BYTES (read per call), at least 1
inline int64_t sc2_chunk_bytes() {
  const char* e = getenv("CS_SC2_CHUNK_BYTES");
  if (!e || !e[0]) return SC2_CHUNK_BYTES;
  const long long v = strtoll(e, nullptr, 10);
  return v >= 1 ? (int64_t)v : SC2_CHUNK_BYTES;
}

// The call as chunks [first, last) of whole problems: as many consecutive problems as fit `limit` matrix bytes (sized by the
// capacities), never fewer than one.  The chunks cover [0, n_prob) in order without a gap.
inline std::vector<std::pair<int, int>> sc2_plan(const int64_t* h_off, int n_prob, int64_t limit) {
  std::vector<std::pair<int, int>> chunks;
  int first = 0;
  int64_t bytes = 0;
  for (int p = 0; p < n_prob; ++p) {
    const int64_t b = sc2_matrix_bytes(h_off[p + 1] - h_off[p]);
    if (p > first && bytes + b > limit) {
      chunks.push_back({first, p});
      first = p;
      bytes = 0;
    }
    bytes += b;
  }
  if (n_prob > 0) chunks.push_back({first, n_prob});
  return chunks;
}

}  // namespace cs
