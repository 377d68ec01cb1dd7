// The host side of cs_sc2_batch under the host sanitizers: the argument checks and the chunk planner of
// corsair_amd/csrc/sc2_plan.h, which is plain C++ and touches no device.  A stand-alone program:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/sc2_plan_check.cpp -o sc2_plan_check
//   ./sc2_plan_check        (prints "sc2_plan_check: ok" and exits 0; a failed check or a sanitizer report exits non-zero)
#include <math.h>
#include <string.h>

#include "../corsair_amd/csrc/sc2_plan.h"

using namespace cs;

static int failures = 0;
#define EXPECT(cond)                                                   \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static int check(const void* src, const void* tgt, const int64_t* off, int n_prob, double tau, double corr, int seeds, int k,
                 const void* T, const void* stat, const void* rmse, const char* word) {
  char msg[256];
  memset(msg, 0, sizeof msg);
  const int rc = sc2_check_args(src, tgt, off, n_prob, tau, corr, seeds, k, T, stat, rmse, msg, sizeof msg);
  if (rc != SC2_OK && word && !strstr(msg, word)) {
    fprintf(stderr, "refusal %d says \"%s\", expected \"%s\"\n", rc, msg, word);
    ++failures;
  }
  return rc;
}

// the chunks cover [0, n_prob) in order without a gap, each fits the limit or holds one problem, and none but the last
// could have taken the problem behind it
static void check_plan(const std::vector<int64_t>& off, int64_t limit) {
  const int n_prob = (int)off.size() - 1;
  const std::vector<std::pair<int, int>> chunks = sc2_plan(off.data(), n_prob, limit);
  int at = 0;
  for (const auto& c : chunks) {
    EXPECT(c.first == at && c.second > c.first && c.second <= n_prob);
    int64_t bytes = 0;
    for (int p = c.first; p < c.second; ++p) bytes += sc2_matrix_bytes(off[p + 1] - off[p]);
    EXPECT(c.second - c.first == 1 || bytes <= limit);
    if (c.second < n_prob) EXPECT(bytes + sc2_matrix_bytes(off[c.second + 1] - off[c.second]) > limit);
    at = c.second;
  }
  EXPECT(at == n_prob);
  EXPECT(n_prob > 0 || chunks.empty());
}

int main() {
  const double nan = NAN, inf = INFINITY;
  const int64_t none[1] = {0}, empty[2] = {0, 0}, one[2] = {0, 4}, bad[2] = {5, 2}, neg[2] = {-1, 2}, most[2] = {7, 32775},
                huge[2] = {0, 32769};
  const int64_t many[5] = {3, 3, 10, 10, 40000};
  char buf[8];
  EXPECT(check(nullptr, nullptr, none, 0, 0.01, 0.1, 0, 20, nullptr, nullptr, nullptr, nullptr) == SC2_OK);
  EXPECT(check(nullptr, nullptr, empty, 1, 0.01, 0.1, 8, 2, buf, buf, buf, nullptr) == SC2_OK);
  EXPECT(check(buf, buf, one, 1, 1e300, 5e-324, INT32_MAX, 64, buf, buf, buf, nullptr) == SC2_OK);
  EXPECT(check(buf, buf, most, 1, 0.01, 0.1, 8, 20, buf, buf, buf, nullptr) == SC2_OK);
  EXPECT(check(nullptr, nullptr, nullptr, 0, 0.01, 0.1, 8, 20, nullptr, nullptr, nullptr, "NULL offset") == SC2_INVALID);
  EXPECT(check(nullptr, nullptr, none, -1, 0.01, 0.1, 8, 20, nullptr, nullptr, nullptr, "negative") == SC2_INVALID);
  EXPECT(check(buf, buf, bad, 1, 0.01, 0.1, 8, 20, buf, buf, buf, "bad pair segment") == SC2_INVALID);
  EXPECT(check(buf, buf, neg, 1, 0.01, 0.1, 8, 20, buf, buf, buf, "bad pair segment") == SC2_INVALID);
  EXPECT(check(buf, buf, huge, 1, 0.01, 0.1, 8, 20, buf, buf, buf, "smaller k_nn") == SC2_UNSUPPORTED);
  EXPECT(check(buf, buf, many, 4, 0.01, 0.1, 8, 20, buf, buf, buf, "problem 3") == SC2_UNSUPPORTED);
  for (double v : {0.0, -0.0, -1.0, nan, inf, -inf}) {
    EXPECT(check(nullptr, nullptr, none, 0, v, 0.1, 8, 20, nullptr, nullptr, nullptr, "compat_dist") == SC2_INVALID);
    EXPECT(check(nullptr, nullptr, none, 0, 0.01, v, 8, 20, nullptr, nullptr, nullptr, "max_corr") == SC2_INVALID);
  }
  for (int v : {-1, INT32_MIN}) EXPECT(check(nullptr, nullptr, none, 0, 0.01, 0.1, v, 20, nullptr, nullptr, nullptr, "n_seeds") == SC2_INVALID);
  for (int v : {1, 0, -1, 65, INT32_MIN, INT32_MAX})
    EXPECT(check(nullptr, nullptr, none, 0, 0.01, 0.1, 8, v, nullptr, nullptr, nullptr, "k_consensus") == SC2_UNSUPPORTED);
  EXPECT(check(nullptr, nullptr, empty, 1, 0.01, 0.1, 8, 20, nullptr, buf, buf, "NULL output") == SC2_INVALID);
  EXPECT(check(nullptr, nullptr, empty, 1, 0.01, 0.1, 8, 20, buf, nullptr, buf, "NULL output") == SC2_INVALID);
  EXPECT(check(nullptr, nullptr, empty, 1, 0.01, 0.1, 8, 20, buf, buf, nullptr, "NULL output") == SC2_INVALID);
  EXPECT(check(nullptr, buf, one, 1, 0.01, 0.1, 8, 20, buf, buf, buf, "d_src") == SC2_INVALID);
  EXPECT(check(buf, nullptr, one, 1, 0.01, 0.1, 8, 20, buf, buf, buf, "d_tgt") == SC2_INVALID);

  EXPECT(sc2_words(0) == 0 && sc2_words(1) == 1 && sc2_words(64) == 1 && sc2_words(65) == 2 && sc2_words(4097) == 65);
  EXPECT(sc2_matrix_bytes(0) == 0 && sc2_matrix_bytes(4097) == 8LL * 4097 * 65 && sc2_matrix_bytes(SC2_MAX_CAP) == 128LL << 20);
  const std::vector<std::vector<int64_t>> tables = {
      {0}, {0, 0}, {0, 0, 0, 0}, {0, 5}, {0, 63, 127, 192, 4289}, {10, 10, 4107, 4107, 8204, 8300},
      {0, 32768, 65536, 98304, 98304, 131072}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10}};
  for (const auto& off : tables)
    for (int64_t limit : {(int64_t)1, (int64_t)8, (int64_t)1024, (int64_t)8 * 4097 * 65, (int64_t)16 * 4097 * 65, SC2_CHUNK_BYTES, (int64_t)INT64_MAX})
      check_plan(off, limit);
  const int64_t big[5] = {0, 32768, 65536, 98304, 131072};
  EXPECT(sc2_plan(big, 4, SC2_CHUNK_BYTES).size() == 2);   // 128 MiB each: two per chunk
  EXPECT(sc2_plan(big, 4, 1).size() == 4);
  EXPECT(sc2_plan(big, 4, INT64_MAX).size() == 1);

  setenv("CS_SC2_CHUNK_BYTES", "12345", 1);
  EXPECT(sc2_chunk_bytes() == 12345);
  for (const char* v : {"", "0", "-5", "abc", "99999999999999999999999999"}) {
    setenv("CS_SC2_CHUNK_BYTES", v, 1);
    const int64_t got = sc2_chunk_bytes();
    EXPECT(got >= 1);
  }
  unsetenv("CS_SC2_CHUNK_BYTES");
  EXPECT(sc2_chunk_bytes() == SC2_CHUNK_BYTES);
  if (failures) {
    fprintf(stderr, "sc2_plan_check: %d failed\n", failures);
    return 1;
  }
  printf("sc2_plan_check: ok\n");
  return 0;
}
