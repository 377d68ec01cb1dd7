// The host side of cs_render_views (view.hip) that needs no device: the argument checks and the chunk planner.  Plain C++,
// no HIP header, so that tools/view_plan_check.cpp can run both under the host sanitizers.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <utility>
#include <vector>

namespace cs {

constexpr int VIEW_MAX_SIDE = 4096;
constexpr int64_t VIEW_CHUNK_BYTES = 256LL << 20;   // depth-buffer bytes per chunk unless CS_VIEW_CHUNK_BYTES says otherwise

// The codes of include/corsair_hip.h (CS_OK, CS_ERR_INVALID, CS_ERR_UNSUPPORTED), restated so that this header stands alone.
constexpr int VIEW_OK = 0, VIEW_INVALID = -1, VIEW_UNSUPPORTED = -5;

inline bool view_positive_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }   // false for NaN

// The refusals of cs_render_views in the order of the header; msg (at least 160 bytes) holds the reason of a refusal.
inline int view_check_args(const void* d_xyz, const int64_t* h_off, int n_seg, const void* d_cam, int width, int height,
                           double focal, double point_size, double depth_tol, const void* d_visible, const void* d_stat,
                           char* msg, size_t msg_len) {
  const char* who = "cs_render_views";
#define VIEW_REFUSE(cond, code, ...)        \
  do {                                      \
    if (!(cond)) {                          \
      snprintf(msg, msg_len, __VA_ARGS__);  \
      return (code);                        \
    }                                       \
  } while (0)
  VIEW_REFUSE(h_off, VIEW_INVALID, "%s: NULL offset table", who);
  VIEW_REFUSE(n_seg >= 0, VIEW_INVALID, "%s: negative segment count", who);
  int64_t rows = 0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    VIEW_REFUSE(h_off[sg] >= 0 && sn >= 0, VIEW_INVALID, "%s: bad segment %d", who, sg);
    VIEW_REFUSE(sn < (1LL << 31), VIEW_UNSUPPORTED, "%s: segment %d has 2^31 rows or more", who, sg);
    rows += sn;
  }
  VIEW_REFUSE(view_positive_finite(focal), VIEW_INVALID, "%s: focal must be positive and finite", who);
  VIEW_REFUSE(view_positive_finite(point_size), VIEW_INVALID, "%s: point_size must be positive and finite", who);
  VIEW_REFUSE(view_positive_finite(depth_tol), VIEW_INVALID, "%s: depth_tol must be positive and finite", who);
  VIEW_REFUSE(width >= 1 && width <= VIEW_MAX_SIDE, VIEW_UNSUPPORTED, "%s: width outside [1, %d]", who, VIEW_MAX_SIDE);
  VIEW_REFUSE(height >= 1 && height <= VIEW_MAX_SIDE, VIEW_UNSUPPORTED, "%s: height outside [1, %d]", who, VIEW_MAX_SIDE);
  VIEW_REFUSE(n_seg == 0 || (d_cam && d_stat), VIEW_INVALID, "%s: NULL d_cam or d_stat", who);
  VIEW_REFUSE(rows == 0 || (d_xyz && d_visible), VIEW_INVALID, "%s: NULL d_xyz or d_visible", who);
#undef VIEW_REFUSE
  return VIEW_OK;
}

// depth-buffer bytes per chunk: CS_VIEW_CHUNK_BYTES (read per call), at least 1
inline int64_t view_chunk_bytes() {
  const char* e = getenv("CS_VIEW_CHUNK_BYTES");
  if (!e || !e[0]) return VIEW_CHUNK_BYTES;
  const long long v = strtoll(e, nullptr, 10);
  return v >= 1 ? (int64_t)v : VIEW_CHUNK_BYTES;
}

// The call as chunks [first, last) of whole segments: as many consecutive segments as fit `limit` bytes of depth buffer
// (8 B x height x width each), never fewer than one.  The chunks cover [0, n_seg) in order without a gap.
inline std::vector<std::pair<int, int>> view_plan(int n_seg, int width, int height, int64_t limit) {
  const int64_t per_seg = 8LL * (int64_t)height * (int64_t)width;
  int64_t fit = limit / per_seg;
  if (fit < 1) fit = 1;
  if (fit > (int64_t)n_seg) fit = n_seg;
  std::vector<std::pair<int, int>> chunks;
  for (int64_t s = 0; s < (int64_t)n_seg; s += fit)
    chunks.push_back({(int)s, (int)(s + fit < (int64_t)n_seg ? s + fit : (int64_t)n_seg)});
  return chunks;
}

}  // namespace cs
