// Feature-matching RANSAC: the mutual filter over two 1-NN lists (cs_corr_mutual) and a RANSAC over the surviving
// pairs with Open3D's two pose checkers, the edge-length checker before the three- or four-pair Horn fit and the distance
// checker after it (cs_ransac_fm_batch).  A third estimator beside cs_ransac_batch and cs_fgr_batch, in a unit of its own: it
// shares horn.h's solver and common.h's generator with the first, restates its canonical residual, and takes nothing else.  The
// specification is the comment of the two calls in include/corsair_hip.h; tests/featmatch_ref.py restates it bit for bit.
//
// The hypotheses of a call are made FM_CHUNK at a time (scratch is bounded by the chunk, not by `iterations`):
//   k_fm_hyp    one lane per hypothesis: gather, edge check, fit, distance check; the VALID ones are appended (t and the twelve
//               doubles of R | t) to the problem's list through one integer atomicAdd.  The append order is arbitrary and reaches
//               nothing: the winner is a maximum over (count, ~t).
//   k_fm_count  k_pl_count's form over that list: 256 listed hypotheses x one slice of the problem's pairs per workgroup, the
//               slice staged through LDS widened to f64 once (48 B per pair), every lane reading the same LDS address (a
//               broadcast), the count in a register, one integer atomicAdd per lane.
//   k_fm_best   the u64 maximum of count << 32 | ~t (the smallest t of the largest count), kept across the chunks.
// then k_fm_pick builds the winner again from its t, k_fm_err sums its fixed-point squared error and k_fm_out writes the rows.
// The sizes of a problem (d_m, the list lengths) are read on the device; the grids come from the host's capacities, so no
// call waits for the device.  Integer atomics only; no thread waits for another; every loop is bounded by an argument or by a
// segment's rows.  FM_HYP, FM_TT, FM_SLICE and FM_CHUNK were chosen after plane.hip and are not tuned.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "horn.h"
#include "nn_common.h"

namespace cs {
namespace {

constexpr int FM_HYP = 256;      // lanes per workgroup everywhere: hypotheses (hyp, count, best), rows (mutual, err)
constexpr int FM_TT = 256;       // pairs per LDS stage of the count kernel (12 288 B as f64)
constexpr int FM_SLICE = 1024;   // pairs per slice unless CS_FM_SLICE says otherwise
constexpr int FM_CHUNK = 8192;   // hypotheses per chunk unless CS_FM_CHUNK says otherwise (a multiple of FM_HYP)
constexpr int FM_MAX_CHUNK = 65536;
constexpr size_t FM_SCRATCH = (size_t)256 << 20;   // the chunk shrinks (to FM_HYP at least) to keep the lists below this

struct FmWork {
  int64_t off;    // first slot of the problem
  int32_t cap;    // its slots
  int32_t prob;
  int32_t r0;     // slots [r0, r1) of the problem, local
  int32_t r1;
};

// per problem, zeroed per call (u64 words)
enum { FM_BEST = 0, FM_ERR, FM_ACC };

struct FmSeg {
  double R[12];   // the winner: element 4a+b = R[a][b], 4a+3 = t[a]
  int32_t found, t, count, m;
};

// The canonical distance chain of the posed source (ransac_count.hip evaluates the same one), restated here so that
// the unit takes nothing from ransac.h:
//   p_c = fma(r_c2, sz, fma(r_c1, sy, fma(r_c0, sx, t_c))),  d_c = p_c - q_c,  |d|^2 = fma(dz, dz, fma(dy, dy, dx dx))
__device__ __forceinline__ double fm_residual2(const double (&R)[12], double sx, double sy, double sz, double qx, double qy,
                                               double qz) {
  const double dx = fma(R[2], sz, fma(R[1], sy, fma(R[0], sx, R[3]))) - qx;
  const double dy = fma(R[6], sz, fma(R[5], sy, fma(R[4], sx, R[7]))) - qy;
  const double dz = fma(R[10], sz, fma(R[9], sy, fma(R[8], sx, R[11]))) - qz;
  return fma(dz, dz, fma(dy, dy, dx * dx));
}

// the pairs of problem p: min(max(d_m[p], 0), capacity), the capacity without d_m
__device__ __forceinline__ int fm_rows(const int32_t* __restrict__ d_m, int p, int cap) {
  return d_m ? min(max(d_m[p], 0), cap) : cap;
}

// Hypothesis t of a problem of m >= 1 pairs (src, tgt: its first rows).  true = valid, R = R | t.
template <int RN>
__device__ __forceinline__ bool fm_hypothesis(const float* __restrict__ src, const float* __restrict__ tgt, uint32_t m,
                                              uint64_t seed, uint32_t t, double sim2, bool edge, bool dist_check, double thr2,
                                              double (&R)[12]) {
  float pa[RN][6];   // the samples as loaded; every widening below is exact
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const int64_t i = rng_index(seed, t, (uint64_t)j, m);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      pa[j][c] = src[3 * i + c];
      pa[j][3 + c] = tgt[3 * i + c];
    }
  }
  if (edge) {
    bool ok = true;
#pragma unroll
    for (int a = 0; a < RN; ++a)
#pragma unroll
      for (int b = a + 1; b < RN; ++b) {
        const double sx = (double)pa[a][0] - (double)pa[b][0], sy = (double)pa[a][1] - (double)pa[b][1],
                     sz = (double)pa[a][2] - (double)pa[b][2];
        const double tx = (double)pa[a][3] - (double)pa[b][3], ty = (double)pa[a][4] - (double)pa[b][4],
                     tz = (double)pa[a][5] - (double)pa[b][5];
        const double ls2 = fma(sz, sz, fma(sy, sy, sx * sx));
        const double lt2 = fma(tz, tz, fma(ty, ty, tx * tx));
        ok = ok && ls2 >= sim2 * lt2 && lt2 >= sim2 * ls2;   // false for NaN
      }
    if (!ok) return false;
  }
  double cs_[3] = {0, 0, 0}, ct_[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < RN; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      cs_[c] += (double)pa[j][c];
      ct_[c] += (double)pa[j][3 + c];
    }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    cs_[c] = cs_[c] / (double)RN;
    ct_[c] = ct_[c] / (double)RN;
  }
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
#pragma unroll
  for (int j = 0; j < RN; ++j) {
    const double ds[3] = {(double)pa[j][0] - cs_[0], (double)pa[j][1] - cs_[1], (double)pa[j][2] - cs_[2]};
    const double dt[3] = {(double)pa[j][3] - ct_[0], (double)pa[j][4] - ct_[1], (double)pa[j][5] - ct_[2]};
#pragma unroll
    for (int x = 0; x < 3; ++x)
#pragma unroll
      for (int y = 0; y < 3; ++y) S[x][y] = fma(ds[x], dt[y], S[x][y]);
  }
  double N[4][4];
  N[0][0] = S[0][0] + S[1][1] + S[2][2];
  N[0][1] = S[1][2] - S[2][1];
  N[0][2] = S[2][0] - S[0][2];
  N[0][3] = S[0][1] - S[1][0];
  N[1][1] = S[0][0] - S[1][1] - S[2][2];
  N[1][2] = S[0][1] + S[1][0];
  N[1][3] = S[2][0] + S[0][2];
  N[2][2] = -S[0][0] + S[1][1] - S[2][2];
  N[2][3] = S[1][2] + S[2][1];
  N[3][3] = -S[0][0] - S[1][1] + S[2][2];
  N[1][0] = N[0][1];
  N[2][0] = N[0][2];
  N[3][0] = N[0][3];
  N[2][1] = N[1][2];
  N[3][1] = N[1][3];
  N[3][2] = N[2][3];
  double qv[4];
  if (!horn_qcp(S, N, qv)) return false;   // no Jacobi here: a fit the solver declines is an invalid hypothesis
  double qw = qv[0], qx = qv[1], qy = qv[2], qz = qv[3];
  const double qn = sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
  qw = qw / qn;
  qx = qx / qn;
  qy = qy / qn;
  qz = qz / qn;
  R[0] = 1.0 - 2.0 * (qy * qy + qz * qz);
  R[1] = 2.0 * (qx * qy - qw * qz);
  R[2] = 2.0 * (qx * qz + qw * qy);
  R[4] = 2.0 * (qx * qy + qw * qz);
  R[5] = 1.0 - 2.0 * (qx * qx + qz * qz);
  R[6] = 2.0 * (qy * qz - qw * qx);
  R[8] = 2.0 * (qx * qz - qw * qy);
  R[9] = 2.0 * (qy * qz + qw * qx);
  R[10] = 1.0 - 2.0 * (qx * qx + qy * qy);
  bool ok = true;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    R[4 * a + 3] = ct_[a] - (R[4 * a] * cs_[0] + R[4 * a + 1] * cs_[1] + R[4 * a + 2] * cs_[2]);
#pragma unroll
    for (int b = 0; b < 4; ++b) ok = ok && fabs(R[4 * a + b]) < INFINITY;   // false for NaN
  }
  if (!ok) return false;
  if (dist_check) {
#pragma unroll
    for (int j = 0; j < RN; ++j)
      ok = ok && fm_residual2(R, (double)pa[j][0], (double)pa[j][1], (double)pa[j][2], (double)pa[j][3], (double)pa[j][4],
                               (double)pa[j][5]) < thr2;
  }
  return ok;
}

struct FmParam {
  double thr2, sim2;
  uint64_t seed;
  int64_t iterations;
  int edge, dist_check, chunk;
};

// grid (chunk / FM_HYP, problems).  list_t / hyp / cnt are [prob][chunk] and [prob][12][chunk]; nvalid is this chunk's row.
template <int RN>
__global__ __launch_bounds__(FM_HYP) void k_fm_hyp(const float* __restrict__ src, const float* __restrict__ tgt,
                                                   const int64_t* __restrict__ off, const int32_t* __restrict__ d_m,
                                                   const FmParam prm, int64_t t0, int32_t* __restrict__ nvalid,
                                                   int32_t* __restrict__ list_t, double* __restrict__ hyp,
                                                   unsigned* __restrict__ cnt) {
  const int p = blockIdx.y;
  const int h = blockIdx.x * FM_HYP + threadIdx.x;   // < chunk: the grid is chunk / FM_HYP wide
  cnt[(int64_t)p * prm.chunk + h] = 0;                // the counts of the previous chunk have been read (stream order)
  const int64_t t = t0 + h;
  if (t >= prm.iterations) return;
  const int64_t o = off[p];
  const int m = fm_rows(d_m, p, (int)(off[p + 1] - o));
  if (m < RN) return;
  double R[12];
  if (!fm_hypothesis<RN>(src + 3 * o, tgt + 3 * o, (uint32_t)m, prm.seed, (uint32_t)t, prm.sim2, prm.edge != 0,
                         prm.dist_check != 0, prm.thr2, R))
    return;
  const int slot = atomicAdd(&nvalid[p], 1);          // < chunk: at most one append per lane of the chunk
  list_t[(int64_t)p * prm.chunk + slot] = (int32_t)t;
  double* hp = hyp + (int64_t)p * 12 * prm.chunk + slot;
#pragma unroll
  for (int e = 0; e < 12; ++e) hp[(int64_t)e * prm.chunk] = R[e];
}

// grid (slices, chunk / FM_HYP)
__global__ __launch_bounds__(FM_HYP) void k_fm_count(const FmWork* __restrict__ work, const float* __restrict__ src,
                                                     const float* __restrict__ tgt, const int32_t* __restrict__ d_m,
                                                     int chunk, double thr2, const int32_t* __restrict__ nvalid,
                                                     const double* __restrict__ hyp, unsigned* __restrict__ cnt) {
  __shared__ double lds[FM_TT][6];
  const FmWork wk = work[blockIdx.x];
  const int m = fm_rows(d_m, wk.prob, wk.cap);
  const int nv = nvalid[wk.prob];
  const int tid = threadIdx.x;
  const int slot = blockIdx.y * FM_HYP + tid;
  const int r1 = min(wk.r1, m);
  if (wk.r0 >= r1 || blockIdx.y * FM_HYP >= nv) return;   // the same for the whole workgroup
  const bool active = slot < nv;
  double R[12];
  {
    const double* hp = hyp + (int64_t)wk.prob * 12 * chunk + (active ? slot : 0);
#pragma unroll
    for (int e = 0; e < 12; ++e) R[e] = hp[(int64_t)e * chunk];
  }
  const float* s = src + 3 * wk.off;
  const float* q = tgt + 3 * wk.off;
  int c = 0;
  for (int base = wk.r0; base < r1; base += FM_TT) {
    const int n = min(FM_TT, r1 - base);
    __syncthreads();
    for (int i = tid; i < n * 3; i += FM_HYP) {
      const int row = i / 3, col = i - 3 * row;
      lds[row][col] = (double)s[(int64_t)base * 3 + i];
      lds[row][3 + col] = (double)q[(int64_t)base * 3 + i];
    }
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < n; ++j) {
      const double* r = lds[j];
      c += fm_residual2(R, r[0], r[1], r[2], r[3], r[4], r[5]) < thr2 ? 1 : 0;   // false for NaN
    }
  }
  if (active && c) atomicAdd(&cnt[(int64_t)wk.prob * chunk + slot], (unsigned)c);
}

// grid (chunk / FM_HYP, problems)
__global__ __launch_bounds__(FM_HYP) void k_fm_best(const unsigned* __restrict__ cnt, const int32_t* __restrict__ list_t,
                                                    const int32_t* __restrict__ nvalid, int chunk,
                                                    unsigned long long* __restrict__ acc) {
  const int p = blockIdx.y;
  const int slot = blockIdx.x * FM_HYP + threadIdx.x;
  unsigned long long key = 0;
  if (slot < nvalid[p]) {
    const int64_t at = (int64_t)p * chunk + slot;
    key = ((unsigned long long)cnt[at] << 32) | (unsigned long long)(~(unsigned)list_t[at]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && (key >> 32)) atomicMax(&acc[FM_ACC * (int64_t)p + FM_BEST], key);
}

// One thread per problem: the winner, built again from its t; d_T.
template <int RN>
__global__ void k_fm_pick(const unsigned long long* __restrict__ acc, const float* __restrict__ src,
                          const float* __restrict__ tgt, const int64_t* __restrict__ off, const int32_t* __restrict__ d_m,
                          int n_prob, const FmParam prm, FmSeg* __restrict__ segs, double* __restrict__ d_T) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  const unsigned long long key = acc[FM_ACC * (int64_t)p + FM_BEST];
  const int64_t o = off[p];
  FmSeg sg = {};
  sg.m = fm_rows(d_m, p, (int)(off[p + 1] - o));
  sg.count = (int32_t)(key >> 32);
  sg.found = sg.m >= RN && sg.count >= RN;
  sg.t = sg.found ? (int32_t)(~(unsigned)(key & 0xffffffffull)) : -1;
  if (sg.found) {
    fm_hypothesis<RN>(src + 3 * o, tgt + 3 * o, (uint32_t)sg.m, prm.seed, (uint32_t)sg.t, prm.sim2, prm.edge != 0,
                      prm.dist_check != 0, prm.thr2, sg.R);
  } else {
    sg.count = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) sg.R[e] = (e % 5 == 0) ? 1.0 : 0.0;
  }
  segs[p] = sg;
  double* T = d_T + 16 * (int64_t)p;
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = sg.R[e];
  T[12] = T[13] = T[14] = 0.0;
  T[15] = 1.0;
}

// k = 61 - eM - ex with m <= 2^eM and thr2 = f 2^ex (ex from the host, clamped there)
__device__ __forceinline__ int fm_shift(int m, int ex) {
  const int eM = m <= 1 ? 0 : 32 - __clz(m - 1);
  return 61 - eM - ex;
}

// The fixed-point squared error of the winner over its inliers: FM_HYP slots per workgroup.
__global__ __launch_bounds__(FM_HYP) void k_fm_err(const FmWork* __restrict__ work, const float* __restrict__ src,
                                                   const float* __restrict__ tgt, const FmSeg* __restrict__ segs, double thr2,
                                                   int ex, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long part[FM_HYP / 64];
  const FmWork wk = work[blockIdx.x];
  const FmSeg* sg = segs + wk.prob;
  if (!sg->found || wk.r0 >= sg->m) return;   // the same for the whole workgroup
  const int row = wk.r0 + threadIdx.x;
  unsigned long long err = 0;
  if (row < wk.r1 && row < sg->m) {
    double R[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) R[e] = sg->R[e];
    const float* s = src + 3 * (wk.off + row);
    const float* q = tgt + 3 * (wk.off + row);
    const double d2 = fm_residual2(R, (double)s[0], (double)s[1], (double)s[2], (double)q[0], (double)q[1], (double)q[2]);
    if (d2 < thr2) err = (unsigned long long)(d2 * ldexp(1.0, fm_shift(sg->m, ex)));   // below 2^(61 - eM)
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) err += __shfl_xor(err, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = err;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long w = 0;
#pragma unroll
    for (int k = 0; k < FM_HYP / 64; ++k) w += part[k];
    if (w) atomicAdd(&acc[FM_ACC * (int64_t)wk.prob + FM_ERR], w);
  }
}

// One thread per problem: d_stat and d_rmse.  nvalid is [n_chunk][n_prob].
__global__ void k_fm_out(const unsigned long long* __restrict__ acc, const FmSeg* __restrict__ segs,
                         const int32_t* __restrict__ nvalid, int n_chunk, int n_prob, int ex, int32_t* __restrict__ d_stat,
                         double* __restrict__ d_rmse) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  const FmSeg* sg = segs + p;
  int64_t nv = 0;
  for (int c = 0; c < n_chunk; ++c) nv += nvalid[(int64_t)c * n_prob + p];
  int32_t* st = d_stat + 4 * (int64_t)p;
  st[0] = sg->found;
  st[1] = sg->t;
  st[2] = sg->count;
  st[3] = (int32_t)nv;
  double rmse = 0.0;
  if (sg->found) {
    const unsigned long long err = acc[FM_ACC * (int64_t)p + FM_ERR];
    rmse = sqrt(((double)err * ldexp(1.0, -fm_shift(sg->m, ex))) / (double)sg->count);
  }
  d_rmse[p] = rmse;
}

// One workgroup per pair: the count of the mutual matches, then the stable compaction of the rows kept.
__global__ __launch_bounds__(FM_HYP) void k_fm_mutual(const int32_t* __restrict__ nn_fwd, const int32_t* __restrict__ nn_bwd,
                                                      const float* __restrict__ xyz0, const float* __restrict__ xyz1,
                                                      const int64_t* __restrict__ off0, const int64_t* __restrict__ off1,
                                                      int ransac_n, int mutual, float* __restrict__ src,
                                                      float* __restrict__ tgt, int32_t* __restrict__ d_m,
                                                      int32_t* __restrict__ d_stat) {
  __shared__ int part[FM_HYP / 64][2];
  const int p = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t a0 = off0[p], b0 = off1[p];
  const int n0 = (int)(off0[p + 1] - a0), n1 = (int)(off1[p + 1] - b0);
  auto match = [&](int i, int& j, bool& valid, bool& mut) {
    j = nn_fwd[a0 + i];
    valid = j >= 0 && j < n1;
    mut = mutual && valid && nn_bwd[b0 + j] == i;   // nn_bwd is not read with the filter off
  };
  int n_valid = 0, n_mut = 0;
  for (int i = tid; i < n0; i += FM_HYP) {
    int j;
    bool valid, mut;
    match(i, j, valid, mut);
    n_valid += valid ? 1 : 0;
    n_mut += mut ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    n_valid += __shfl_xor(n_valid, o);
    n_mut += __shfl_xor(n_mut, o);
  }
  if (lane == 0) {
    part[wave][0] = n_valid;
    part[wave][1] = n_mut;
  }
  __syncthreads();
  n_valid = n_mut = 0;
#pragma unroll
  for (int k = 0; k < FM_HYP / 64; ++k) {
    n_valid += part[k][0];
    n_mut += part[k][1];
  }
  const bool use_mut = mutual && n_mut >= 3 * ransac_n;
  int base = 0;   // rows kept so far: the same in every thread
  for (int c0 = 0; c0 < n0; c0 += FM_HYP) {
    const int i = c0 + tid;
    int j = 0;
    bool valid = false, mut = false;
    if (i < n0) match(i, j, valid, mut);
    const bool keep = use_mut ? mut : valid;
    const unsigned long long b = __ballot(keep);
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();   // part of the previous round (or of the count) has been read
    if (lane == 0) part[wave][0] = __popcll(b);
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int k = 0; k < FM_HYP / 64; ++k) {
      woff += k < wave ? part[k][0] : 0;
      total += part[k][0];
    }
    if (keep) {
      const int64_t slot = a0 + base + woff + before;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        src[3 * slot + c] = xyz0[3 * (a0 + i) + c];
        tgt[3 * slot + c] = xyz1[3 * (b0 + j) + c];
      }
    }
    base += total;
  }
  for (int i = base + tid; i < n0; i += FM_HYP) {   // the slots past the count are zero, not stale
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      src[3 * (a0 + i) + c] = 0.f;
      tgt[3 * (a0 + i) + c] = 0.f;
    }
  }
  if (tid == 0) {
    d_m[p] = base;
    d_stat[2 * p] = mutual ? n_mut : n_valid;
    d_stat[2 * p + 1] = (mutual && !use_mut) ? 1 : 0;
  }
}

// a positive value of an environment variable (read per call), else the default
int64_t env_rows(const char* name, int64_t dflt) {
  const char* e = getenv(name);
  if (!e || !e[0]) return dflt;
  const long v = strtol(e, nullptr, 10);
  return v >= 1 && v < (1L << 31) ? (int64_t)v : dflt;
}

void push_rows(std::vector<FmWork>& work, int64_t off, int64_t cap, int prob, int64_t step) {
  for (int64_t r = 0; r < cap; r += step)
    work.push_back(FmWork{off, (int32_t)cap, (int32_t)prob, (int32_t)r, (int32_t)std::min(cap, r + step)});
}

// the offset table of a call: CS_OK and the rows, or the refusal
int check_offsets(const char* who, const char* what, const int64_t* h_off, int n, int64_t& rows) {
  rows = 0;
  for (int p = 0; p < n; ++p) {
    const int64_t sn = h_off[p + 1] - h_off[p];
    CS_REQUIRE(h_off[p] >= 0 && sn >= 0, CS_ERR_INVALID, "%s: bad %s segment %d", who, what, p);
    CS_REQUIRE(sn < (1LL << 31), CS_ERR_UNSUPPORTED, "%s: %s segment %d has 2^31 rows or more", who, what, p);
    rows += sn;
  }
  return CS_OK;
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_corr_mutual(const int32_t* d_nn_fwd, const int32_t* d_nn_bwd, const float* d_xyz0, const int64_t* h_off0,
                   const float* d_xyz1, const int64_t* h_off1, int n_pair, int ransac_n, int mutual, float* d_src,
                   float* d_tgt, int32_t* d_m, int32_t* d_stat, void* stream) {
  const char* who = "cs_corr_mutual";
  CS_REQUIRE(h_off0 && h_off1, CS_ERR_INVALID, "%s: NULL offset table", who);
  CS_REQUIRE(n_pair >= 0, CS_ERR_INVALID, "%s: negative pair count", who);
  int64_t rows0 = 0, rows1 = 0;
  int rc = check_offsets(who, "query", h_off0, n_pair, rows0);
  if (!rc) rc = check_offsets(who, "CAD", h_off1, n_pair, rows1);
  if (rc) return rc;
  CS_REQUIRE(ransac_n >= 1 && ransac_n <= (1 << 20), CS_ERR_INVALID, "%s: ransac_n outside [1, 2^20]", who);
  CS_REQUIRE(mutual == 0 || mutual == 1, CS_ERR_INVALID, "%s: mutual must be 0 or 1", who);
  if (n_pair == 0) return CS_OK;
  CS_REQUIRE(d_m && d_stat, CS_ERR_INVALID, "%s: NULL argument", who);
  CS_REQUIRE(rows0 == 0 || (d_nn_fwd && d_xyz0 && d_src && d_tgt), CS_ERR_INVALID, "%s: NULL argument", who);
  CS_REQUIRE(rows0 == 0 || rows1 == 0 || (d_xyz1 && (d_nn_bwd || !mutual)), CS_ERR_INVALID, "%s: NULL argument", who);
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  std::vector<int64_t> off(h_off0, h_off0 + n_pair + 1);
  off.insert(off.end(), h_off1, h_off1 + n_pair + 1);
  PoolBuf<int64_t> d_off;
  rc = upload(d_off, off, s);
  if (rc) return rc;
  ProfScope prof("featmatch", s, 2.0 * (double)rows0);
  hipLaunchKernelGGL(k_fm_mutual, dim3((unsigned)n_pair), dim3(FM_HYP), 0, s, d_nn_fwd, d_nn_bwd, d_xyz0, d_xyz1,
                     (const int64_t*)d_off.p, (const int64_t*)d_off.p + n_pair + 1, ransac_n, mutual, d_src, d_tgt, d_m,
                     d_stat);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

int cs_ransac_fm_batch(const float* d_src, const float* d_tgt, const int64_t* h_off, const int32_t* d_m, int n_prob,
                       double max_corr, int ransac_n, double edge_similarity, int check_distance, int64_t iterations,
                       uint64_t seed, double* d_T, int32_t* d_stat, double* d_rmse, void* stream) {
  const char* who = "cs_ransac_fm_batch";
  CS_REQUIRE(h_off, CS_ERR_INVALID, "%s: NULL offset table", who);
  CS_REQUIRE(n_prob >= 0, CS_ERR_INVALID, "%s: negative problem count", who);
  int64_t rows = 0;
  int rc = check_offsets(who, "pair", h_off, n_prob, rows);
  if (rc) return rc;
  CS_REQUIRE(max_corr > 0.0 && max_corr <= 1.7976931348623157e308, CS_ERR_INVALID,
             "%s: max_corr must be positive and finite", who);
  CS_REQUIRE(edge_similarity >= 0.0 && edge_similarity <= 1.0, CS_ERR_INVALID, "%s: edge_similarity outside [0, 1]", who);
  CS_REQUIRE(iterations >= 1, CS_ERR_INVALID, "%s: iterations below 1", who);
  CS_REQUIRE(iterations < (1LL << 31), CS_ERR_UNSUPPORTED, "%s: 2^31 iterations or more", who);
  CS_REQUIRE(ransac_n == 3 || ransac_n == 4, CS_ERR_UNSUPPORTED, "%s: ransac_n must be 3 or 4", who);
  if (n_prob == 0) return CS_OK;
  CS_REQUIRE(d_T && d_stat && d_rmse, CS_ERR_INVALID, "%s: NULL argument", who);
  CS_REQUIRE(rows == 0 || (d_src && d_tgt), CS_ERR_INVALID, "%s: NULL argument", who);
  FmParam prm;
  prm.thr2 = max_corr * max_corr;   // +inf or 0 for a max_corr beyond 1.3e154 or below 1.5e-162
  prm.sim2 = edge_similarity * edge_similarity;
  prm.seed = seed;
  prm.iterations = iterations;
  prm.edge = edge_similarity > 0.0;
  prm.dist_check = check_distance != 0;
  int ex = 1024;
  if (prm.thr2 <= 1.7976931348623157e308) {
    frexp(prm.thr2, &ex);
    ex = std::max(ex, -900);
  }
  // hypotheses per chunk: a multiple of FM_HYP, no more than the call needs, small enough for the scratch bound
  int64_t chunk = std::min<int64_t>(env_rows("CS_FM_CHUNK", FM_CHUNK), FM_MAX_CHUNK);
  chunk = std::min(chunk, iterations);
  const int64_t fit = (int64_t)(FM_SCRATCH / ((size_t)n_prob * 108));
  chunk = std::max<int64_t>(ceil_div(std::min(chunk, std::max<int64_t>(fit, 1)), FM_HYP) * FM_HYP, FM_HYP);
  prm.chunk = (int)chunk;
  const int n_chunk = (int)ceil_div(iterations, chunk), tiles = (int)(chunk / FM_HYP);
  const int64_t slice = env_rows("CS_FM_SLICE", FM_SLICE);
  std::vector<FmWork> slices, blocks;
  std::vector<int64_t> off(h_off, h_off + n_prob + 1);
  for (int p = 0; p < n_prob; ++p) {
    const int64_t cap = h_off[p + 1] - h_off[p];
    push_rows(slices, h_off[p], cap, p, slice);
    push_rows(blocks, h_off[p], cap, p, FM_HYP);
  }
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const size_t n_list = (size_t)n_prob * (size_t)chunk, n_acc = (size_t)FM_ACC * n_prob,
               n_nv = (size_t)n_chunk * (size_t)n_prob;
  PoolBuf<FmWork> d_slices, d_blocks;
  PoolBuf<int64_t> d_off;
  PoolBuf<unsigned> cnt(n_list);
  PoolBuf<int32_t> list_t(n_list), nvalid(n_nv);
  PoolBuf<double> hyp(12 * n_list);
  PoolBuf<unsigned long long> acc(n_acc);
  PoolBuf<FmSeg> segs((size_t)n_prob);
  CS_REQUIRE(cnt.p && list_t.p && nvalid.p && hyp.p && acc.p && segs.p, CS_ERR_HIP, "%s: scratch allocation failed", who);
  rc = upload(d_off, off, s);
  if (!rc && rows > 0) rc = upload(d_slices, slices, s);
  if (!rc && rows > 0) rc = upload(d_blocks, blocks, s);
  if (rc) return rc;
  CS_HIP_CHECK(hipMemsetAsync(nvalid.p, 0, n_nv * sizeof(int32_t), s));
  CS_HIP_CHECK(hipMemsetAsync(acc.p, 0, n_acc * sizeof(unsigned long long), s));
  ProfScope prof("featmatch", s, 400.0 * (double)n_prob * (double)iterations);
  const dim3 block(FM_HYP), g_hyp((unsigned)tiles, (unsigned)n_prob), g_prob((unsigned)ceil_div(n_prob, 256));
  const auto hyp_kernel = ransac_n == 3 ? k_fm_hyp<3> : k_fm_hyp<4>;
  const auto pick_kernel = ransac_n == 3 ? k_fm_pick<3> : k_fm_pick<4>;
  if (rows > 0) {
    for (int c = 0; c < n_chunk; ++c) {
      int32_t* nv = nvalid.p + (size_t)c * n_prob;
      hipLaunchKernelGGL(hyp_kernel, g_hyp, block, 0, s, d_src, d_tgt, (const int64_t*)d_off.p, d_m, prm, (int64_t)c * chunk,
                         nv, list_t.p, hyp.p, cnt.p);
      hipLaunchKernelGGL(k_fm_count, dim3((unsigned)slices.size(), (unsigned)tiles), block, 0, s, (const FmWork*)d_slices.p,
                         d_src, d_tgt, d_m, prm.chunk, prm.thr2, (const int32_t*)nv, (const double*)hyp.p, cnt.p);
      hipLaunchKernelGGL(k_fm_best, g_hyp, block, 0, s, (const unsigned*)cnt.p, (const int32_t*)list_t.p, (const int32_t*)nv,
                         prm.chunk, acc.p);
    }
  }
  hipLaunchKernelGGL(pick_kernel, g_prob, dim3(256), 0, s, (const unsigned long long*)acc.p, d_src, d_tgt,
                     (const int64_t*)d_off.p, d_m, n_prob, prm, segs.p, d_T);
  if (rows > 0)
    hipLaunchKernelGGL(k_fm_err, dim3((unsigned)blocks.size()), block, 0, s, (const FmWork*)d_blocks.p, d_src, d_tgt,
                       (const FmSeg*)segs.p, prm.thr2, ex, acc.p);
  hipLaunchKernelGGL(k_fm_out, g_prob, dim3(256), 0, s, (const unsigned long long*)acc.p, (const FmSeg*)segs.p,
                     (const int32_t*)nvalid.p, n_chunk, n_prob, ex, d_stat, d_rmse);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // extern "C"
