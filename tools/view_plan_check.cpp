// The host side of cs_render_views under the host sanitizers: the argument checks and the chunk planner of
// corsair_amd/csrc/view_plan.h, which is plain C++ and touches no device.  A stand-alone program:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/view_plan_check.cpp -o view_plan_check
//   ./view_plan_check        (prints "view_plan_check: ok" and exits 0; a failed check or a sanitizer report exits non-zero)
#include <math.h>
#include <string.h>

#include "../corsair_amd/csrc/view_plan.h"

using namespace cs;

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static int check(const void* xyz, const int64_t* off, int n_seg, const void* cam, int w, int h, double focal, double ps,
                 double tol, const void* vis, const void* stat, const char* word) {
  char msg[160];
  memset(msg, 0, sizeof msg);
  const int rc = view_check_args(xyz, off, n_seg, cam, w, h, focal, ps, tol, vis, stat, msg, sizeof msg);
  if (rc != VIEW_OK && word && !strstr(msg, word)) {
    fprintf(stderr, "refusal %d says \"%s\", expected \"%s\"\n", rc, msg, word);
    ++failures;
  }
  return rc;
}

// the chunks cover [0, n_seg) in order without a gap, each fits the limit or holds one segment
static void check_plan(int n_seg, int w, int h, int64_t limit) {
  const std::vector<std::pair<int, int>> chunks = view_plan(n_seg, w, h, limit);
  const int64_t per_seg = 8LL * h * w;
  int at = 0;
  for (const auto& c : chunks) {
    EXPECT(c.first == at && c.second > c.first && c.second <= n_seg);
    const int64_t segs = c.second - c.first;
    EXPECT(segs == 1 || segs * per_seg <= limit);
    at = c.second;
  }
  EXPECT(at == n_seg);
  EXPECT(n_seg > 0 || chunks.empty());
  if (n_seg > 0 && limit >= per_seg) {   // no chunk but the last is smaller than what fits
    const int64_t fit = limit / per_seg < n_seg ? limit / per_seg : n_seg;
    for (size_t i = 0; i + 1 < chunks.size(); ++i) EXPECT(chunks[i].second - chunks[i].first == fit);
  }
}

int main() {
  const double nan = NAN, inf = INFINITY;
  const int64_t none[1] = {0}, empty[2] = {0, 0}, one[2] = {0, 4}, bad[2] = {5, 2}, neg[2] = {-1, 2}, huge[2] = {0, 1LL << 31};
  const int64_t many[5] = {3, 3, 10, 10, 2147483700LL};
  char buf[8];
  EXPECT(check(nullptr, none, 0, nullptr, 8, 8, 8.0, 0.1, 0.1, nullptr, nullptr, nullptr) == VIEW_OK);
  EXPECT(check(nullptr, empty, 1, buf, 1, 1, 8.0, 0.1, 0.1, nullptr, buf, nullptr) == VIEW_OK);
  EXPECT(check(buf, one, 1, buf, 4096, 4096, 1e300, 1e-300, 5e-324, buf, buf, nullptr) == VIEW_OK);
  EXPECT(check(nullptr, nullptr, 0, nullptr, 8, 8, 8.0, 0.1, 0.1, nullptr, nullptr, "NULL offset") == VIEW_INVALID);
  EXPECT(check(nullptr, none, -1, nullptr, 8, 8, 8.0, 0.1, 0.1, nullptr, nullptr, "negative") == VIEW_INVALID);
  EXPECT(check(buf, bad, 1, buf, 8, 8, 8.0, 0.1, 0.1, buf, buf, "bad segment") == VIEW_INVALID);
  EXPECT(check(buf, neg, 1, buf, 8, 8, 8.0, 0.1, 0.1, buf, buf, "bad segment") == VIEW_INVALID);
  EXPECT(check(buf, huge, 1, buf, 8, 8, 8.0, 0.1, 0.1, buf, buf, "2^31") == VIEW_UNSUPPORTED);
  EXPECT(check(buf, many, 4, buf, 8, 8, 8.0, 0.1, 0.1, buf, buf, "segment 3") == VIEW_UNSUPPORTED);
  for (double v : {0.0, -0.0, -1.0, nan, inf, -inf}) {
    EXPECT(check(nullptr, none, 0, nullptr, 8, 8, v, 0.1, 0.1, nullptr, nullptr, "focal") == VIEW_INVALID);
    EXPECT(check(nullptr, none, 0, nullptr, 8, 8, 8.0, v, 0.1, nullptr, nullptr, "point_size") == VIEW_INVALID);
    EXPECT(check(nullptr, none, 0, nullptr, 8, 8, 8.0, 0.1, v, nullptr, nullptr, "depth_tol") == VIEW_INVALID);
  }
  for (int v : {0, -1, 4097, INT32_MIN, INT32_MAX}) {
    EXPECT(check(nullptr, none, 0, nullptr, v, 8, 8.0, 0.1, 0.1, nullptr, nullptr, "width") == VIEW_UNSUPPORTED);
    EXPECT(check(nullptr, none, 0, nullptr, 8, v, 8.0, 0.1, 0.1, nullptr, nullptr, "height") == VIEW_UNSUPPORTED);
  }
  EXPECT(check(nullptr, empty, 1, nullptr, 8, 8, 8.0, 0.1, 0.1, nullptr, buf, "d_cam") == VIEW_INVALID);
  EXPECT(check(nullptr, empty, 1, buf, 8, 8, 8.0, 0.1, 0.1, nullptr, nullptr, "d_stat") == VIEW_INVALID);
  EXPECT(check(nullptr, one, 1, buf, 8, 8, 8.0, 0.1, 0.1, buf, buf, "d_xyz") == VIEW_INVALID);
  EXPECT(check(buf, one, 1, buf, 8, 8, 8.0, 0.1, 0.1, nullptr, buf, "d_visible") == VIEW_INVALID);

  for (int n_seg : {0, 1, 2, 7, 32, 1000, 65537})
    for (int side : {1, 7, 256, 4096})
      for (int64_t limit : {(int64_t)1, (int64_t)8, (int64_t)8 * side * side, (int64_t)8 * side * side * 3 + 5, VIEW_CHUNK_BYTES,
                            (int64_t)INT64_MAX})
        check_plan(n_seg, side, side == 7 ? 5 : side, limit);
  EXPECT(view_plan(32, 256, 256, VIEW_CHUNK_BYTES).size() == 1);
  EXPECT(view_plan(32, 512, 512, 8LL * 512 * 512 * 8).size() == 4);
  EXPECT(view_plan(3, 4096, 4096, VIEW_CHUNK_BYTES).size() == 2);   // 128 MiB each: two per chunk

  setenv("CS_VIEW_CHUNK_BYTES", "12345", 1);
  EXPECT(view_chunk_bytes() == 12345);
  for (const char* v : {"", "0", "-5", "abc", "99999999999999999999999999"}) {
    setenv("CS_VIEW_CHUNK_BYTES", v, 1);
    const int64_t got = view_chunk_bytes();
    EXPECT(got >= 1);
  }
  unsetenv("CS_VIEW_CHUNK_BYTES");
  EXPECT(view_chunk_bytes() == VIEW_CHUNK_BYTES);
  if (failures) {
    fprintf(stderr, "view_plan_check: %d failed\n", failures);
    return 1;
  }
  printf("view_plan_check: ok\n");
  return 0;
}
