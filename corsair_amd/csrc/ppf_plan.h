// The host side of cs_ppf_batch (ppf.hip) that needs no device: the argument checks, the accumulator rule and the chunk
// planner.  Plain C++, no HIP header, so that tools/ppf_plan_check.cpp can run them under the host sanitizers (sc2_plan.h's
// pattern).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

namespace cs {

constexpr int PPF_MAX_MODEL = 4096;                 // rows of a model segment: its table holds m^2 entries of 12 B (192 MiB)
constexpr int PPF_MAX_SCENE = 16384;                // rows of a scene segment
constexpr int PPF_MAX_CAND = 64;                    // n_cand
constexpr int PPF_DIST_BINS = 64, PPF_ANGLE_BINS = 15, PPF_ALPHA_BINS = 30;
constexpr int PPF_KEYS = PPF_DIST_BINS * PPF_ANGLE_BINS * PPF_ANGLE_BINS * PPF_ANGLE_BINS;   // 216 000
constexpr int PPF_LDS_ROWS = 1360;                  // model rows whose 30 counters each fit the LDS of a CU (163 200 B of 160 KiB)
constexpr int PPF_SLABS = 256;                      // workgroups of the global-slab voting launch, one slab each
constexpr int64_t PPF_CHUNK_BYTES = 512LL << 20;    // table and slab bytes per chunk unless CS_PPF_CHUNK_BYTES says otherwise

// The codes of include/corsair_hip.h (CS_OK, CS_ERR_INVALID, CS_ERR_UNSUPPORTED), restated so that this header stands alone.
constexpr int PPF_OK = 0, PPF_INVALID = -1, PPF_UNSUPPORTED = -5;

inline bool ppf_positive_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }   // false for NaN

// bytes of one model table of m rows: m^2 entries (row, y, z) and two int32 arrays over the keys (counts, starts)
inline int64_t ppf_table_bytes(int64_t m) { return 12 * m * m + 8 * ((int64_t)PPF_KEYS + 1); }
// bytes of the global accumulator slabs a problem of m model rows asks for: none when its counters fit the LDS
inline int64_t ppf_slab_bytes(int64_t m, int lds_rows) { return m > lds_rows ? (int64_t)PPF_SLABS * 4 * PPF_ALPHA_BINS * m : 0; }
inline int64_t ppf_problem_bytes(int64_t m, int lds_rows) { return ppf_table_bytes(m) + ppf_slab_bytes(m, lds_rows); }

// The refusals of cs_ppf_batch in the order of the header; msg (at least 200 bytes) holds the reason of a refusal.
inline int ppf_check_args(const void* d_scene, const void* d_scene_normal, const int64_t* h_soff, const void* d_model,
                          const void* d_model_normal, const int64_t* h_moff, const int32_t* h_scene_seg,
                          const int32_t* h_model_seg, int n_prob, const double* h_dist_step, double max_dist, int ref_step,
                          int n_cand, const void* d_T, const void* d_Tinv, const void* d_stat, const void* d_rmse,
                          const void* d_cand_T, const void* d_cand_stat, char* msg, size_t msg_len) {
  const char* who = "cs_ppf_batch";
#define PPF_REFUSE(cond, code, ...)         \
  do {                                      \
    if (!(cond)) {                          \
      snprintf(msg, msg_len, __VA_ARGS__);  \
      return (code);                        \
    }                                       \
  } while (0)
  PPF_REFUSE(n_prob >= 0, PPF_INVALID, "%s: negative problem count", who);
  PPF_REFUSE(n_prob == 0 || (h_soff && h_moff && h_scene_seg && h_model_seg && h_dist_step), PPF_INVALID,
             "%s: NULL host table", who);
  int64_t s_rows = 0, m_rows = 0;
  for (int p = 0; p < n_prob; ++p) {
    PPF_REFUSE(h_scene_seg[p] >= 0 && h_model_seg[p] >= 0, PPF_INVALID, "%s: negative segment id in problem %d", who, p);
    const int64_t s0 = h_soff[h_scene_seg[p]], s1 = h_soff[h_scene_seg[p] + 1];
    const int64_t m0 = h_moff[h_model_seg[p]], m1 = h_moff[h_model_seg[p] + 1];
    PPF_REFUSE(s0 >= 0 && s1 >= s0, PPF_INVALID, "%s: bad scene segment in problem %d", who, p);
    PPF_REFUSE(m0 >= 0 && m1 >= m0, PPF_INVALID, "%s: bad model segment in problem %d", who, p);
    s_rows += s1 - s0;
    m_rows += m1 - m0;
  }
  for (int p = 0; p < n_prob; ++p)
    PPF_REFUSE(ppf_positive_finite(h_dist_step[p]), PPF_INVALID, "%s: dist_step of problem %d must be positive and finite", who,
               p);
  PPF_REFUSE(ppf_positive_finite(max_dist), PPF_INVALID, "%s: max_dist must be positive and finite", who);
  PPF_REFUSE(ref_step >= 1, PPF_INVALID, "%s: ref_step must be at least 1", who);
  PPF_REFUSE(n_cand >= 1 && n_cand <= PPF_MAX_CAND, PPF_UNSUPPORTED, "%s: n_cand outside [1, %d]", who, PPF_MAX_CAND);
  for (int p = 0; p < n_prob; ++p) {
    PPF_REFUSE(h_moff[h_model_seg[p] + 1] - h_moff[h_model_seg[p]] <= PPF_MAX_MODEL, PPF_UNSUPPORTED,
               "%s: the model of problem %d has more than %d rows (its table of all ordered pairs would exceed 192 MiB): "
               "sample it with a coarser voxel",
               who, p, PPF_MAX_MODEL);
    PPF_REFUSE(h_soff[h_scene_seg[p] + 1] - h_soff[h_scene_seg[p]] <= PPF_MAX_SCENE, PPF_UNSUPPORTED,
               "%s: the scene of problem %d has more than %d rows: sample it with a coarser voxel", who, p, PPF_MAX_SCENE);
  }
  PPF_REFUSE(n_prob == 0 || (d_T && d_Tinv && d_stat && d_rmse && d_cand_T && d_cand_stat), PPF_INVALID, "%s: NULL output",
             who);
  PPF_REFUSE(s_rows == 0 || (d_scene && d_scene_normal), PPF_INVALID, "%s: NULL d_scene or d_scene_normal", who);
  PPF_REFUSE(m_rows == 0 || (d_model && d_model_normal), PPF_INVALID, "%s: NULL d_model or d_model_normal", who);
#undef PPF_REFUSE
  return PPF_OK;
}

// table and slab bytes per chunk: CS_PPF_CHUNK_BYTES (read per call), at least 1
inline int64_t ppf_chunk_bytes() {
  const char* e = getenv("CS_PPF_CHUNK_BYTES");
  if (!e || !e[0]) return PPF_CHUNK_BYTES;
  const long long v = strtoll(e, nullptr, 10);
  return v >= 1 ? (int64_t)v : PPF_CHUNK_BYTES;
}

// The model rows up to which a problem's accumulator lives in the LDS: CS_PPF_ACC (read per call) = "global" sends every
// problem to the zeroed global slabs (0), "lds" or nothing is the rule of the header (PPF_LDS_ROWS).
inline int ppf_lds_rows() {
  const char* e = getenv("CS_PPF_ACC");
  return e && e[0] == 'g' ? 0 : PPF_LDS_ROWS;
}

// The call as chunks [first, last) of whole problems: as many consecutive problems as fit `limit` bytes (every problem
// counted with a table of its own, which is the most it can need), never fewer than one.  The chunks cover [0, n_prob) in
// order without a gap.
inline std::vector<std::pair<int, int>> ppf_plan(const int64_t* h_moff, const int32_t* h_model_seg, int n_prob, int lds_rows,
                                                 int64_t limit) {
  std::vector<std::pair<int, int>> chunks;
  int first = 0;
  int64_t bytes = 0;
  for (int p = 0; p < n_prob; ++p) {
    const int64_t b = ppf_problem_bytes(h_moff[h_model_seg[p] + 1] - h_moff[h_model_seg[p]], lds_rows);
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
