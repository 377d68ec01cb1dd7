// The host side of cs_ppf_batch under the host sanitizers: the argument checks, the accumulator rule and the chunk
// planner of corsair_amd/csrc/ppf_plan.h, which is plain C++ and touches no device.  A stand-alone program:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ppf_plan_check.cpp -o ppf_plan_check
//   ./ppf_plan_check        (prints "ppf_plan_check: ok" and exits 0; a failed check or a sanitizer report exits non-zero)
#include <math.h>
#include <string.h>

#include "../corsair_amd/csrc/ppf_plan.h"

using namespace cs;

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

struct Call {
  const void* arrays;
  const int64_t *soff, *moff;
  const int32_t *sseg, *mseg;
  int n_prob;
  const double* step;
  double max_dist;
  int ref_step, n_cand;
  const void* out;
};

static int check(const Call& c, const char* word) {
  char msg[320];
  memset(msg, 0, sizeof msg);
  const int rc = ppf_check_args(c.arrays, c.arrays, c.soff, c.arrays, c.arrays, c.moff, c.sseg, c.mseg, c.n_prob, c.step,
                                c.max_dist, c.ref_step, c.n_cand, c.out, c.out, c.out, c.out, c.out, c.out, msg, sizeof msg);
  if (rc != PPF_OK && word && !strstr(msg, word)) {
    fprintf(stderr, "refusal %d says \"%s\", expected \"%s\"\n", rc, msg, word);
    ++failures;
  }
  return rc;
}

// the chunks cover [0, n_prob) in order without a gap, each fits the limit or holds one problem, and none but the last
// could have taken the problem behind it
static void check_plan(const std::vector<int64_t>& moff, const std::vector<int32_t>& seg, int lds_rows, int64_t limit) {
  const int n_prob = (int)seg.size();
  const std::vector<std::pair<int, int>> chunks = ppf_plan(moff.data(), seg.data(), n_prob, lds_rows, limit);
  auto bytes_of = [&](int p) { return ppf_problem_bytes(moff[seg[p] + 1] - moff[seg[p]], lds_rows); };
  int at = 0;
  for (const auto& c : chunks) {
    EXPECT(c.first == at && c.second > c.first && c.second <= n_prob);
    int64_t bytes = 0;
    for (int p = c.first; p < c.second; ++p) bytes += bytes_of(p);
    EXPECT(c.second - c.first == 1 || bytes <= limit);
    if (c.second < n_prob) EXPECT(bytes + bytes_of(c.second) > limit);
    at = c.second;
  }
  EXPECT(at == n_prob);
  EXPECT(n_prob > 0 || chunks.empty());
}

int main() {
  const double nan = NAN, inf = INFINITY;
  char buf[8];
  const int64_t off[3] = {0, 4, 9}, bad[2] = {5, 2}, neg[2] = {-1, 2}, m_most[2] = {7, 4103}, m_huge[2] = {0, 4097},
                s_most[2] = {3, 16387}, s_huge[2] = {0, 16385}, empty[2] = {0, 0};
  const int32_t seg0[2] = {0, 1}, seg_neg[1] = {-1};
  const double step[2] = {0.05, 1e300};
  const Call ok = {buf, off, off, seg0, seg0, 2, step, 0.1, 5, 16, buf};
  EXPECT(check(ok, nullptr) == PPF_OK);
  Call c = ok;
  c.n_prob = 0, c.soff = c.moff = nullptr, c.sseg = c.mseg = nullptr, c.step = nullptr, c.out = c.arrays = nullptr;
  EXPECT(check(c, nullptr) == PPF_OK);
  c = ok, c.n_prob = -1;
  EXPECT(check(c, "negative problem count") == PPF_INVALID);
  for (int k = 0; k < 5; ++k) {
    c = ok;
    if (k == 0) c.soff = nullptr;
    if (k == 1) c.moff = nullptr;
    if (k == 2) c.sseg = nullptr;
    if (k == 3) c.mseg = nullptr;
    if (k == 4) c.step = nullptr;
    EXPECT(check(c, "NULL host table") == PPF_INVALID);
  }
  c = ok, c.n_prob = 1, c.sseg = seg_neg;
  EXPECT(check(c, "negative segment id") == PPF_INVALID);
  c = ok, c.n_prob = 1, c.mseg = seg_neg;
  EXPECT(check(c, "negative segment id") == PPF_INVALID);
  c = ok, c.n_prob = 1, c.soff = bad;
  EXPECT(check(c, "bad scene segment") == PPF_INVALID);
  c = ok, c.n_prob = 1, c.moff = neg;
  EXPECT(check(c, "bad model segment") == PPF_INVALID);
  for (double v : {0.0, -0.0, -1.0, nan, inf, -inf}) {
    const double s2[2] = {0.05, v};
    c = ok, c.step = s2;
    EXPECT(check(c, "dist_step of problem 1") == PPF_INVALID);
    c = ok, c.max_dist = v;
    EXPECT(check(c, "max_dist") == PPF_INVALID);
  }
  for (int v : {0, -1, INT32_MIN}) {
    c = ok, c.ref_step = v;
    EXPECT(check(c, "ref_step") == PPF_INVALID);
  }
  c = ok, c.ref_step = INT32_MAX;
  EXPECT(check(c, nullptr) == PPF_OK);
  for (int v : {0, -1, 65, INT32_MIN, INT32_MAX}) {
    c = ok, c.n_cand = v;
    EXPECT(check(c, "n_cand") == PPF_UNSUPPORTED);
  }
  for (int v : {1, 64}) {
    c = ok, c.n_cand = v;
    EXPECT(check(c, nullptr) == PPF_OK);
  }
  c = ok, c.n_prob = 1, c.moff = m_most, c.soff = s_most;
  EXPECT(check(c, nullptr) == PPF_OK);
  c = ok, c.n_prob = 1, c.moff = m_huge;
  EXPECT(check(c, "coarser voxel") == PPF_UNSUPPORTED);
  c = ok, c.n_prob = 1, c.soff = s_huge;
  EXPECT(check(c, "scene of problem 0") == PPF_UNSUPPORTED);
  c = ok, c.out = nullptr;
  EXPECT(check(c, "NULL output") == PPF_INVALID);
  c = ok, c.arrays = nullptr;
  EXPECT(check(c, "d_scene") == PPF_INVALID);
  c = ok, c.arrays = nullptr, c.n_prob = 1, c.soff = empty;
  EXPECT(check(c, "d_model") == PPF_INVALID);
  c = ok, c.arrays = nullptr, c.n_prob = 1, c.soff = empty, c.moff = empty;
  EXPECT(check(c, nullptr) == PPF_OK);

  EXPECT(PPF_KEYS == 216000 && 4 * PPF_ALPHA_BINS * PPF_LDS_ROWS + 16 <= 160 * 1024);
  EXPECT(ppf_table_bytes(0) == 8 * 216001 && ppf_table_bytes(PPF_MAX_MODEL) == (192LL << 20) + 8 * 216001);
  EXPECT(ppf_slab_bytes(PPF_LDS_ROWS, PPF_LDS_ROWS) == 0 && ppf_slab_bytes(PPF_LDS_ROWS + 1, PPF_LDS_ROWS) == 256LL * 120 * 1361);
  EXPECT(ppf_slab_bytes(1, 0) == 256 * 120 && ppf_slab_bytes(0, 0) == 0);
  const std::vector<int64_t> moff = {0, 0, 1, 65, 365, 1065, 2565, 6661};
  const std::vector<std::vector<int32_t>> segs = {{}, {0}, {0, 0, 0}, {6}, {0, 1, 2, 3, 4, 5, 6}, {6, 6, 5, 4, 4, 3, 0, 6}, {3, 3, 3, 3, 3, 3}};
  for (const auto& seg : segs)
    for (int lds_rows : {PPF_LDS_ROWS, 0})
      for (int64_t limit : {(int64_t)1, (int64_t)8 * 216001, ppf_problem_bytes(300, lds_rows), 2 * ppf_problem_bytes(300, lds_rows),
                            ppf_problem_bytes(4096, lds_rows), PPF_CHUNK_BYTES, (int64_t)INT64_MAX})
        check_plan(moff, seg, lds_rows, limit);
  const std::vector<int32_t> four = {3, 3, 3, 3};
  EXPECT(ppf_plan(moff.data(), four.data(), 4, PPF_LDS_ROWS, 1).size() == 4);
  EXPECT(ppf_plan(moff.data(), four.data(), 4, PPF_LDS_ROWS, 2 * ppf_problem_bytes(300, PPF_LDS_ROWS)).size() == 2);
  EXPECT(ppf_plan(moff.data(), four.data(), 4, PPF_LDS_ROWS, INT64_MAX).size() == 1);

  setenv("CS_PPF_CHUNK_BYTES", "12345", 1);
  EXPECT(ppf_chunk_bytes() == 12345);
  for (const char* v : {"", "0", "-5", "abc", "99999999999999999999999999"}) {
    setenv("CS_PPF_CHUNK_BYTES", v, 1);
    EXPECT(ppf_chunk_bytes() >= 1);
  }
  unsetenv("CS_PPF_CHUNK_BYTES");
  EXPECT(ppf_chunk_bytes() == PPF_CHUNK_BYTES);
  EXPECT(ppf_lds_rows() == PPF_LDS_ROWS);
  setenv("CS_PPF_ACC", "global", 1);
  EXPECT(ppf_lds_rows() == 0);
  for (const char* v : {"lds", "", "x"}) {
    setenv("CS_PPF_ACC", v, 1);
    EXPECT(ppf_lds_rows() == PPF_LDS_ROWS);
  }
  unsetenv("CS_PPF_ACC");
  if (failures) {
    fprintf(stderr, "ppf_plan_check: %d failed\n", failures);
    return 1;
  }
  printf("ppf_plan_check: ok\n");
  return 0;
}
