// Support-plane segmentation of raw scans: a fixed number of three-row plane hypotheses per segment, counted
// against every row, the best one refitted over its inliers by an order-free fixed-point covariance, and the final inlier
// mask with the plane oriented towards the side the rows lie on.  The specification is the comment of cs_segment_plane in
// include/corsair_hip.h; tests/plane_ref.py restates it bit for bit.
//
// k_pl_count is the hot kernel: one workgroup = PL_HYP hypotheses of one segment x one slice of its rows.  Every thread
// builds its own hypothesis into registers (three gathers; origin, normal and bound: seven doubles), the slice goes through
// LDS PL_TT rows at a time, widened to f64 ONCE while it is staged (the widening is exact, so the bits are those of the
// header's "(double) row"), and every lane reads the same LDS address per row: a broadcast.  The count stays in a register
// and ends in one integer atomicAdd into cnt[seg][t].  Everything after it is a per-row pass or one thread per segment.
// Integer atomics only (sums, maxima); no thread waits for another; every loop is bounded by iters or the segment's rows.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "horn.h"
#include "nn_common.h"

namespace cs {
namespace {

constexpr int PL_HYP = 256;    // hypotheses per workgroup of the count kernel, rows per workgroup of the row passes
constexpr int PL_TT = 512;     // slice rows per LDS stage (12 288 B as f64)
constexpr int PL_SLICE = 1024; // rows per slice unless CS_PLANE_SLICE says otherwise.  Not tuned.
constexpr int PL_MAX_ITERS = 65536;

struct PlWork {
  int64_t seg0;   // first row of the segment (global)
  int32_t sn;     // rows of the segment
  int32_t seg;    // the segment
  int32_t r0;     // rows [r0, r1) of the segment, local
  int32_t r1;
};

// Per segment, zeroed per call.  u64 words: the rest of the record is written by the per-segment kernels.
enum {
  PL_BEST = 0,     // count << 32 | ~t of the best hypothesis
  PL_M,            // bit pattern of M
  PL_SUM,          // nine signed sums (two's complement): S_x S_y S_z S_xx S_xy S_xz S_yy S_yz S_zz
  PL_FINAL = PL_SUM + 9,   // final inliers
  PL_POS,
  PL_NEG,
  PL_FINITE,
  PL_ACC
};

struct PlSeg {
  double o[3];      // p_i0 of the best hypothesis
  double ns[3];     // its normal, not normalised
  double nn;
  double bound;
  double n[3];      // the final plane before the orientation
  double c[3];
  int32_t found, t, count, refit;
};

// Hypothesis t of a segment: origin, normal and bound; bound = 0 (nothing is strictly below it) when it is not valid.
__device__ __forceinline__ void pl_hypothesis(const float* __restrict__ seg, uint32_t m, uint64_t seed, uint32_t t,
                                              double thr2, double (&o)[3], double (&n)[3], double& nn, double& bound) {
  const uint32_t i0 = rng_index(seed, t, 0, m), i1 = rng_index(seed, t, 1, m), i2 = rng_index(seed, t, 2, m);
  double a[3], b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    o[c] = (double)seg[3 * (int64_t)i0 + c];
    a[c] = (double)seg[3 * (int64_t)i1 + c] - o[c];
    b[c] = (double)seg[3 * (int64_t)i2 + c] - o[c];
  }
  n[0] = fma(a[1], b[2], -(a[2] * b[1]));
  n[1] = fma(a[2], b[0], -(a[0] * b[2]));
  n[2] = fma(a[0], b[1], -(a[1] * b[0]));
  nn = fma(n[2], n[2], fma(n[1], n[1], n[0] * n[0]));
  const double bd = thr2 * nn;
  const bool valid = nn > 0.0 && nn < INFINITY && bd > 0.0 && bd < INFINITY;   // false for NaN
  bound = valid ? bd : 0.0;
}

// s of a row (x, y, z) against the plane through c with normal n
__device__ __forceinline__ double pl_s(double x, double y, double z, const double (&c)[3], const double (&n)[3]) {
  const double ux = x - c[0], uy = y - c[1], uz = z - c[2];
  return fma(uz, n[2], fma(uy, n[1], ux * n[0]));
}

__global__ __launch_bounds__(PL_HYP) void k_pl_count(const PlWork* __restrict__ work, const float* __restrict__ xyz,
                                                     int iters, uint64_t seed, double thr2, unsigned* __restrict__ cnt) {
  __shared__ double t_lds[PL_TT * 3];
  const PlWork wk = work[blockIdx.x];
  const int tid = threadIdx.x;
  const int t = blockIdx.y * PL_HYP + tid;
  const bool active = t < iters;
  const float* seg = xyz + wk.seg0 * 3;
  double o[3] = {0, 0, 0}, n[3] = {0, 0, 0}, nn = 0, bound = 0;
  if (active) pl_hypothesis(seg, (uint32_t)wk.sn, seed, (uint32_t)t, thr2, o, n, nn, bound);
  int c = 0;
  for (int tbase = wk.r0; tbase < wk.r1; tbase += PL_TT) {
    const int tcount = min(PL_TT, wk.r1 - tbase);
    __syncthreads();
    for (int i = tid; i < tcount * 3; i += PL_HYP) t_lds[i] = (double)seg[(int64_t)tbase * 3 + i];
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < tcount; ++j) {
      const double s = pl_s(t_lds[3 * j], t_lds[3 * j + 1], t_lds[3 * j + 2], o, n);
      c += s * s < bound ? 1 : 0;   // false for NaN
    }
  }
  if (active && c) atomicAdd(&cnt[(int64_t)wk.seg * iters + t], (unsigned)c);
}

// One workgroup = PL_HYP hypotheses of one segment: the maximum of count << 32 | ~t (the smallest t of the largest count).
__global__ __launch_bounds__(PL_HYP) void k_pl_best(const unsigned* __restrict__ cnt, int iters, int tiles,
                                                    unsigned long long* __restrict__ acc) {
  const int seg = blockIdx.x / tiles;
  const int t = (blockIdx.x % tiles) * PL_HYP + threadIdx.x;
  unsigned long long key = 0;
  if (t < iters) key = ((unsigned long long)cnt[(int64_t)seg * iters + t] << 32) | (unsigned long long)(~(unsigned)t);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && key) atomicMax(&acc[PL_ACC * (int64_t)seg + PL_BEST], key);
}

// One thread per segment: the best hypothesis, built again from its t.
__global__ void k_pl_pick(const unsigned long long* __restrict__ acc, const float* __restrict__ xyz,
                          const int64_t* __restrict__ off, int n_seg, uint64_t seed, double thr2, PlSeg* __restrict__ segs) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_seg) return;
  const unsigned long long key = acc[PL_ACC * (int64_t)p + PL_BEST];
  PlSeg sg = {};
  sg.count = (int32_t)(key >> 32);
  sg.found = sg.count >= 3;
  sg.t = sg.found ? (int32_t)(~(unsigned)(key & 0xffffffffull)) : -1;
  if (sg.found) {
    const int64_t seg0 = off[p];
    pl_hypothesis(xyz + seg0 * 3, (uint32_t)(off[p + 1] - seg0), seed, (uint32_t)sg.t, thr2, sg.o, sg.ns, sg.nn, sg.bound);
  } else {
    sg.count = 0;
  }
  segs[p] = sg;
}

__device__ __forceinline__ bool pl_load(const PlWork& wk, const float* __restrict__ xyz, int row, double& x, double& y,
                                        double& z) {
  if (row >= wk.r1) return false;
  const float* r = xyz + (wk.seg0 + row) * 3;
  x = (double)r[0];
  y = (double)r[1];
  z = (double)r[2];
  return true;
}

// The stage-1 mask of the best hypothesis (into inlier, which stage 3 overwrites) and M.
__global__ __launch_bounds__(PL_HYP) void k_pl_mask(const PlWork* __restrict__ work, const float* __restrict__ xyz,
                                                    const PlSeg* __restrict__ segs, uint8_t* __restrict__ inlier,
                                                    unsigned long long* __restrict__ acc) {
  const PlWork wk = work[blockIdx.x];
  const PlSeg* sg = segs + wk.seg;
  if (!sg->found) return;   // the same for the whole workgroup
  const int row = wk.r0 + threadIdx.x;
  double x = 0, y = 0, z = 0;
  const bool have = pl_load(wk, xyz, row, x, y, z);
  bool in = false;
  unsigned long long bits = 0;
  if (have) {
    const double o[3] = {sg->o[0], sg->o[1], sg->o[2]}, n[3] = {sg->ns[0], sg->ns[1], sg->ns[2]};
    const double s = pl_s(x, y, z, o, n);
    in = s * s < sg->bound;
    inlier[wk.seg0 + row] = in ? 1 : 0;
    if (in) {   // u is finite here: an infinite u gives an infinite or NaN s
      const double ax = fabs(x - o[0]), ay = fabs(y - o[1]), az = fabs(z - o[2]);
      const double mx = ax > ay ? ax : ay;
      bits = (unsigned long long)__double_as_longlong(mx > az ? mx : az);
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(bits, o);
    bits = other > bits ? other : bits;
  }
  if ((threadIdx.x & 63) == 0 && bits) atomicMax(&acc[PL_ACC * (int64_t)wk.seg + PL_M], bits);
}

// sh = min(15 - e, 1023) for M = f 2^e, f in [0.5, 1)
__device__ __forceinline__ int pl_shift(double M) {
  int e = 0;
  frexp(M, &e);
  return min(15 - e, 1023);
}

__device__ __forceinline__ unsigned long long pl_wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// v[0..N) summed over the workgroup (wave shuffles, then LDS), one atomicAdd per value by the threads 0..N-1
template <int N>
__device__ __forceinline__ void pl_block_add(unsigned long long (&v)[N], unsigned long long* __restrict__ dst) {
  __shared__ unsigned long long part[PL_HYP / 64][N];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const unsigned long long w = pl_wave_sum(v[i]);
    if (lane == 0) part[wave][i] = w;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    unsigned long long w = 0;
#pragma unroll
    for (int k = 0; k < PL_HYP / 64; ++k) w += part[k][threadIdx.x];
    if (w) atomicAdd(&dst[threadIdx.x], w);
  }
}

// The nine integer sums over the stage-1 inliers.
__global__ __launch_bounds__(PL_HYP) void k_pl_sums(const PlWork* __restrict__ work, const float* __restrict__ xyz,
                                                    const PlSeg* __restrict__ segs, const uint8_t* __restrict__ inlier,
                                                    unsigned long long* __restrict__ acc) {
  const PlWork wk = work[blockIdx.x];
  const PlSeg* sg = segs + wk.seg;
  unsigned long long* a = acc + PL_ACC * (int64_t)wk.seg;
  const double M = __longlong_as_double((long long)a[PL_M]);
  if (!sg->found || !(M > 0.0)) return;   // the same for the whole workgroup
  const int sh = pl_shift(M);
  const int row = wk.r0 + threadIdx.x;
  double x = 0, y = 0, z = 0;
  long long q0 = 0, q1 = 0, q2 = 0;
  if (pl_load(wk, xyz, row, x, y, z) && inlier[wk.seg0 + row]) {
    q0 = (long long)rint(ldexp(x - sg->o[0], sh));   // |q| <= 2^15
    q1 = (long long)rint(ldexp(y - sg->o[1], sh));
    q2 = (long long)rint(ldexp(z - sg->o[2], sh));
  }
  unsigned long long v[9] = {(unsigned long long)q0,        (unsigned long long)q1,        (unsigned long long)q2,
                             (unsigned long long)(q0 * q0), (unsigned long long)(q0 * q1), (unsigned long long)(q0 * q2),
                             (unsigned long long)(q1 * q1), (unsigned long long)(q1 * q2), (unsigned long long)(q2 * q2)};
  pl_block_add<9>(v, a + PL_SUM);
}

// n S_ab - S_a S_b in 128 bits, to f64: the magnitude as (double)hi * 2^64 + (double)lo, then the sign
__device__ __forceinline__ double pl_cov(long long n, long long sab, long long sa, long long sb) {
  const __int128 c = (__int128)n * (__int128)sab - (__int128)sa * (__int128)sb;
  const bool neg = c < 0;
  const unsigned __int128 mag = neg ? (unsigned __int128)0 - (unsigned __int128)c : (unsigned __int128)c;
  const double d = (double)(unsigned long long)(mag >> 64) * 0x1.0p64 + (double)(unsigned long long)mag;
  return neg ? -d : d;
}

// One thread per segment: the refit, or the sampled plane where it is skipped.
__global__ void k_pl_fit(const unsigned long long* __restrict__ acc, int n_seg, PlSeg* __restrict__ segs) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_seg) return;
  PlSeg* sg = segs + p;
  if (!sg->found) return;
  const unsigned long long* a = acc + PL_ACC * (int64_t)p;
  const double M = __longlong_as_double((long long)a[PL_M]);
  bool refit = false;
  double e0 = 0, e1 = 0, e2 = 0, len2 = 0;
  if (M > 0.0) {
    const long long n = sg->count;
    const long long s0 = (long long)a[PL_SUM + 0], s1 = (long long)a[PL_SUM + 1], s2 = (long long)a[PL_SUM + 2];
    double c[3][3], v[3][3];
    c[0][0] = pl_cov(n, (long long)a[PL_SUM + 3], s0, s0);
    c[0][1] = pl_cov(n, (long long)a[PL_SUM + 4], s0, s1);
    c[0][2] = pl_cov(n, (long long)a[PL_SUM + 5], s0, s2);
    c[1][1] = pl_cov(n, (long long)a[PL_SUM + 6], s1, s1);
    c[1][2] = pl_cov(n, (long long)a[PL_SUM + 7], s1, s2);
    c[2][2] = pl_cov(n, (long long)a[PL_SUM + 8], s2, s2);
    c[1][0] = c[0][1];
    c[2][0] = c[0][2];
    c[2][1] = c[1][2];
    jacobi3(c, v);
    // the column of the smallest diagonal entry (ties -> the smaller column), value by value as nrm_finish selects it
    const double w0 = c[0][0], w1 = c[1][1], w2 = c[2][2];
    const bool c1 = w1 < w0;
    const double best = c1 ? w1 : w0;
    const bool c2 = w2 < best;
    e0 = c2 ? v[0][2] : (c1 ? v[0][1] : v[0][0]);
    e1 = c2 ? v[1][2] : (c1 ? v[1][1] : v[1][0]);
    e2 = c2 ? v[2][2] : (c1 ? v[2][1] : v[2][0]);
    len2 = fma(e2, e2, fma(e1, e1, e0 * e0));
    refit = len2 > 0.0 && len2 < INFINITY;   // false for NaN; a finite len2 has finite components
    if (refit) {
      const int sh = pl_shift(M);
      const double dn = (double)n;
      sg->c[0] = sg->o[0] + ldexp((double)s0 / dn, -sh);
      sg->c[1] = sg->o[1] + ldexp((double)s1 / dn, -sh);
      sg->c[2] = sg->o[2] + ldexp((double)s2 / dn, -sh);
    }
  }
  if (!refit) {
    e0 = sg->ns[0];
    e1 = sg->ns[1];
    e2 = sg->ns[2];
    len2 = sg->nn;
    sg->c[0] = sg->o[0];
    sg->c[1] = sg->o[1];
    sg->c[2] = sg->o[2];
  }
  const double len = sqrt(len2);
  sg->n[0] = e0 / len;
  sg->n[1] = e1 / len;
  sg->n[2] = e2 / len;
  sg->refit = refit ? 1 : 0;
}

// Stage 3: the final mask and the four counts.  Runs for every segment: rows_finite is reported without a plane too.
__global__ __launch_bounds__(PL_HYP) void k_pl_final(const PlWork* __restrict__ work, const float* __restrict__ xyz,
                                                     const PlSeg* __restrict__ segs, double thr2,
                                                     uint8_t* __restrict__ inlier, unsigned long long* __restrict__ acc) {
  const PlWork wk = work[blockIdx.x];
  const PlSeg* sg = segs + wk.seg;
  const int row = wk.r0 + threadIdx.x;
  double x = 0, y = 0, z = 0;
  const bool have = pl_load(wk, xyz, row, x, y, z);
  const bool fin = have && fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY;   // false for NaN
  bool in = false, pos = false, neg = false;
  if (fin && sg->found) {
    const double c[3] = {sg->c[0], sg->c[1], sg->c[2]}, n[3] = {sg->n[0], sg->n[1], sg->n[2]};
    const double s = pl_s(x, y, z, c, n);
    in = s * s < thr2;
    pos = !in && s > 0.0;
    neg = !in && s < 0.0;
  }
  if (have) inlier[wk.seg0 + row] = in ? 1 : 0;
  unsigned long long v[4] = {in ? 1ull : 0ull, pos ? 1ull : 0ull, neg ? 1ull : 0ull, fin ? 1ull : 0ull};
  pl_block_add<4>(v, acc + PL_ACC * (int64_t)wk.seg + PL_FINAL);
}

// One thread per segment: the orientation, d, and the two output rows.
__global__ void k_pl_out(const unsigned long long* __restrict__ acc, const PlSeg* __restrict__ segs, int n_seg,
                         double* __restrict__ plane, int32_t* __restrict__ stat) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_seg) return;
  const PlSeg* sg = segs + p;
  const unsigned long long* a = acc + PL_ACC * (int64_t)p;
  double* pl = plane + 4 * (int64_t)p;
  int32_t* st = stat + 8 * (int64_t)p;
  const int32_t finite = (int32_t)a[PL_FINITE];
  if (!sg->found) {
    pl[0] = pl[1] = pl[2] = pl[3] = 0.0;
    st[0] = 0;
    st[1] = -1;
    st[2] = st[3] = st[4] = st[5] = st[6] = 0;
    st[7] = finite;
    return;
  }
  double n0 = sg->n[0], n1 = sg->n[1], n2 = sg->n[2];
  int32_t n_pos = (int32_t)a[PL_POS], n_neg = (int32_t)a[PL_NEG];
  bool flip = n_neg > n_pos;
  if (n_neg == n_pos) {   // cs_estimate_normals' rule: the component of largest magnitude (the first on ties) is positive
    double big = fabs(n0), lead = n0;
    if (fabs(n1) > big) { big = fabs(n1); lead = n1; }
    if (fabs(n2) > big) { big = fabs(n2); lead = n2; }
    flip = lead < 0.0;
  }
  if (flip) {
    n0 = -n0;
    n1 = -n1;
    n2 = -n2;
    const int32_t w = n_pos;
    n_pos = n_neg;
    n_neg = w;
  }
  pl[0] = n0;
  pl[1] = n1;
  pl[2] = n2;
  pl[3] = -fma(sg->c[2], n2, fma(sg->c[1], n1, sg->c[0] * n0));
  st[0] = 1;
  st[1] = sg->t;
  st[2] = sg->count;
  st[3] = sg->refit;
  st[4] = (int32_t)a[PL_FINAL];
  st[5] = n_pos;
  st[6] = n_neg;
  st[7] = finite;
}

// rows per slice of the count kernel: CS_PLANE_SLICE (read per call), at least 1
int slice_rows() {
  const char* e = getenv("CS_PLANE_SLICE");
  if (!e || !e[0]) return PL_SLICE;
  const long v = strtol(e, nullptr, 10);
  return v >= 1 && v < (1L << 31) ? (int)v : PL_SLICE;
}

void push_rows(std::vector<PlWork>& work, int64_t seg0, int64_t sn, int seg, int64_t step) {
  for (int64_t r = 0; r < sn; r += step)
    work.push_back(PlWork{seg0, (int32_t)sn, (int32_t)seg, (int32_t)r, (int32_t)std::min(sn, r + step)});
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_segment_plane(const float* d_xyz, const int64_t* h_off, int n_seg, double dist, int iters, uint64_t seed,
                     double* d_plane, int32_t* d_stat, uint8_t* d_inlier, void* stream) {
  const char* who = "cs_segment_plane";
  CS_REQUIRE(h_off, CS_ERR_INVALID, "%s: NULL offset table", who);
  CS_REQUIRE(n_seg >= 0, CS_ERR_INVALID, "%s: negative segment count", who);
  int64_t rows = 0;
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    CS_REQUIRE(h_off[sg] >= 0 && sn >= 0, CS_ERR_INVALID, "%s: bad segment %d", who, sg);
    CS_REQUIRE(sn < (1LL << 31), CS_ERR_UNSUPPORTED, "%s: segment %d has 2^31 rows or more", who, sg);
    rows += sn;
  }
  CS_REQUIRE(dist > 0.0 && dist <= 1.7976931348623157e308, CS_ERR_INVALID, "%s: dist must be positive and finite", who);
  CS_REQUIRE(iters >= 1 && iters <= PL_MAX_ITERS, CS_ERR_INVALID, "%s: iters outside [1, 65536]", who);
  if (n_seg == 0) return CS_OK;
  CS_REQUIRE(d_plane && d_stat, CS_ERR_INVALID, "%s: NULL argument", who);
  CS_REQUIRE(rows == 0 || (d_xyz && d_inlier), CS_ERR_INVALID, "%s: NULL argument", who);
  const double thr2 = dist * dist;   // +inf or 0 for a dist beyond 1.3e154 or below 1.5e-162: no hypothesis is valid
  const int tiles = (int)ceil_div(iters, PL_HYP);
  const int64_t slice = slice_rows();
  std::vector<PlWork> slices, blocks;
  std::vector<int64_t> off(h_off, h_off + n_seg + 1);
  for (int sg = 0; sg < n_seg; ++sg) {
    const int64_t sn = h_off[sg + 1] - h_off[sg];
    push_rows(slices, h_off[sg], sn, sg, slice);
    push_rows(blocks, h_off[sg], sn, sg, PL_HYP);
  }
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const size_t n_cnt = (size_t)n_seg * (size_t)iters, n_acc = (size_t)PL_ACC * n_seg;
  PoolBuf<PlWork> d_slices, d_blocks;
  PoolBuf<int64_t> d_off;
  PoolBuf<unsigned> cnt(n_cnt);
  PoolBuf<unsigned long long> acc(n_acc);
  PoolBuf<PlSeg> segs((size_t)n_seg);
  CS_REQUIRE(cnt.p && acc.p && segs.p, CS_ERR_HIP, "%s: scratch allocation failed", who);
  int rc = upload(d_off, off, s);
  if (!rc && rows > 0) rc = upload(d_slices, slices, s);
  if (!rc && rows > 0) rc = upload(d_blocks, blocks, s);
  if (rc) return rc;
  CS_HIP_CHECK(hipMemsetAsync(cnt.p, 0, n_cnt * sizeof(unsigned), s));
  CS_HIP_CHECK(hipMemsetAsync(acc.p, 0, n_acc * sizeof(unsigned long long), s));
  ProfScope prof("plane", s, 10.0 * (double)rows * (double)iters);
  const dim3 block(PL_HYP), g_rows((unsigned)blocks.size()), g_seg((unsigned)ceil_div(n_seg, 256));
  if (rows > 0)
    hipLaunchKernelGGL(k_pl_count, dim3((unsigned)slices.size(), (unsigned)tiles), block, 0, s, (const PlWork*)d_slices.p,
                       d_xyz, iters, seed, thr2, cnt.p);
  hipLaunchKernelGGL(k_pl_best, dim3((unsigned)((int64_t)n_seg * tiles)), block, 0, s, (const unsigned*)cnt.p, iters, tiles,
                     acc.p);
  hipLaunchKernelGGL(k_pl_pick, g_seg, dim3(256), 0, s, (const unsigned long long*)acc.p, d_xyz, (const int64_t*)d_off.p,
                     n_seg, seed, thr2, segs.p);
  if (rows > 0) {
    hipLaunchKernelGGL(k_pl_mask, g_rows, block, 0, s, (const PlWork*)d_blocks.p, d_xyz, (const PlSeg*)segs.p, d_inlier,
                       acc.p);
    hipLaunchKernelGGL(k_pl_sums, g_rows, block, 0, s, (const PlWork*)d_blocks.p, d_xyz, (const PlSeg*)segs.p,
                       (const uint8_t*)d_inlier, acc.p);
  }
  hipLaunchKernelGGL(k_pl_fit, g_seg, dim3(256), 0, s, (const unsigned long long*)acc.p, n_seg, segs.p);
  if (rows > 0)
    hipLaunchKernelGGL(k_pl_final, g_rows, block, 0, s, (const PlWork*)d_blocks.p, d_xyz, (const PlSeg*)segs.p, thr2,
                       d_inlier, acc.p);
  hipLaunchKernelGGL(k_pl_out, g_seg, dim3(256), 0, s, (const unsigned long long*)acc.p, (const PlSeg*)segs.p, n_seg,
                     d_plane, d_stat);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // extern "C"
