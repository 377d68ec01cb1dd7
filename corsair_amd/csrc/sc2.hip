// The compatibility-graph correspondence estimator: cs_sc2_batch.  A fourth estimator beside cs_ransac_batch,
// cs_fgr_batch and cs_ransac_fm_batch, in a unit of its own: it shares horn.h's solver with them, restates the canonical
// residual and the fixed-point rmse of featmatch.hip, and takes nothing else.  The specification is the comment of the call in
// include/corsair_hip.h; tests/sc2_ref.py restates it bit for bit.  The argument checks and the chunk planner stand in
// sc2_plan.h (plain C++).
//
// Per chunk of whole problems (their bit matrices, sized by the capacities, fit CS_SC2_CHUNK_BYTES):
//   k_sc2_build  one wave per (row tile I, a span of word columns J >= I): a lane owns row i and walks the 64 wave-uniform rows
//                of a column, forming one u64 word in registers; the tile below the diagonal is the transpose of that word
//                tile (64 ballots).  Degrees through one integer atomicAdd per word.
//   k_sc2_rank   the rank of every row by counting larger keys; the rows of rank < S are the seeds.
//   k_sc2_score  one wave per seed: the second-order count of every set bit of its row (AND + popcount over the words, a
//                wave reduction), the K largest keys kept sorted across the lanes, the consensus set written in ascending row
//                index.
//   k_sc2_fit    one thread per seed: the fit over its consensus set.
//   k_sc2_count  featmatch.hip's count: 256 seeds x one slice of the problem's pairs per workgroup.
//   k_sc2_best   the u64 maximum of count << 32 | ~rank.
// then, once per call, k_sc2_pick reads the winner, k_sc2_err sums its fixed-point squared error and writes the mask, and
// k_sc2_out writes the rows.  The sizes of a problem (d_m) are read on the device; the grids come from the host's capacities,
// so no call waits for the device.  Integer atomics only; no thread waits for another; every loop is bounded by an argument or
// by a problem's rows.  The shapes are first choices and not tuned.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "horn.h"
#include "nn_common.h"
#include "sc2_plan.h"

namespace cs {
namespace {

static_assert(SC2_OK == CS_OK && SC2_INVALID == CS_ERR_INVALID && SC2_UNSUPPORTED == CS_ERR_UNSUPPORTED,
              "sc2_plan.h restates the codes of corsair_hip.h");

constexpr int SC_BLOCK = 256;     // lanes per workgroup of the row and seed kernels
constexpr int SC_TT = 256;        // pairs per LDS stage of the count kernel (12 288 B as f64)
constexpr int SC_SLICE = 1024;    // pairs per slice of the count kernel unless CS_SC2_SLICE says otherwise
constexpr int SC_SPAN = 8;        // word columns per wave of the build kernel unless CS_SC2_SPAN says otherwise
constexpr int SC_SET = SC2_MAX_K + 1;                 // slots of a consensus set
constexpr int SC_ROW_REGS = SC2_MAX_CAP / 64 / 64;    // words of a seed's row per lane of the score kernel (8)

struct ScProb {
  int64_t off;     // first slot of the problem
  int64_t mat;     // first word of its matrix in the chunk's buffer
  int64_t soff;    // first seed slot of the problem (seed slots: min(n_seeds, capacity), the capacity with n_seeds = 0)
  int32_t cap;     // its slots
  int32_t W;       // words per matrix row
};

struct ScWork {
  int32_t prob, a, b, c;   // build: row tile a, word columns [b, c); elsewhere: rows or seeds [a, b)
};

// per problem, zeroed per call (u64 words)
enum { SC_BEST = 0, SC_ERR, SC_NVALID, SC_ACC };

struct ScSeg {
  double R[12];   // the winner: element 4a+b = R[a][b], 4a+3 = t[a]
  int32_t found, row, count, m, rank, deg;
};

// The canonical distance chain of the posed source, as featmatch.hip restates it.
__device__ __forceinline__ double sc_residual2(const double (&R)[12], double sx, double sy, double sz, double qx, double qy,
                                               double qz) {
  const double dx = fma(R[2], sz, fma(R[1], sy, fma(R[0], sx, R[3]))) - qx;
  const double dy = fma(R[6], sz, fma(R[5], sy, fma(R[4], sx, R[7]))) - qy;
  const double dz = fma(R[10], sz, fma(R[9], sy, fma(R[8], sx, R[11]))) - qz;
  return fma(dz, dz, fma(dy, dy, dx * dx));
}

__device__ __forceinline__ int sc_rows(const int32_t* __restrict__ d_m, int p, int cap) {
  return d_m ? min(max(d_m[p], 0), cap) : cap;
}

__device__ __forceinline__ int sc_seeds(int n_seeds, int m) { return n_seeds == 0 ? m : min(n_seeds, m); }

__device__ __forceinline__ bool sc_finite3(double x, double y, double z) {
  return fabs(x) < INFINITY && fabs(y) < INFINITY && fabs(z) < INFINITY;   // false for NaN
}

__device__ __forceinline__ unsigned long long sc_uniform(unsigned long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

// grid (work items), one wave each
__global__ __launch_bounds__(64) void k_sc2_build(const ScWork* __restrict__ work, const ScProb* __restrict__ probs,
                                                  const float* __restrict__ src, const float* __restrict__ tgt,
                                                  const int32_t* __restrict__ d_m, double tau2,
                                                  unsigned long long* __restrict__ mat, int32_t* __restrict__ deg) {
  const ScWork wk = work[blockIdx.x];
  const ScProb pb = probs[wk.prob];
  const int m = sc_rows(d_m, wk.prob, pb.cap);
  const int lane = threadIdx.x;
  const int i = wk.a * 64 + lane;
  const float* s = src + 3 * pb.off;
  const float* q = tgt + 3 * pb.off;
  unsigned long long* M = mat + pb.mat;
  int32_t* dg = deg + pb.off;
  double six = 0, siy = 0, siz = 0, qix = 0, qiy = 0, qiz = 0;
  if (i < m) {
    six = (double)s[3 * i], siy = (double)s[3 * i + 1], siz = (double)s[3 * i + 2];
    qix = (double)q[3 * i], qiy = (double)q[3 * i + 1], qiz = (double)q[3 * i + 2];
  }
  const bool row_ok = i < m && sc_finite3(six, siy, siz) && sc_finite3(qix, qiy, qiz);
  for (int J = wk.b; J < wk.c; ++J) {
    unsigned long long w = 0;
    const int nj = min(64, m - J * 64);   // the same in every lane; <= 0 behind the pairs
    for (int jj = 0; jj < nj; ++jj) {
      const int j = J * 64 + jj;
      const double sjx = (double)s[3 * j], sjy = (double)s[3 * j + 1], sjz = (double)s[3 * j + 2];
      const double qjx = (double)q[3 * j], qjy = (double)q[3 * j + 1], qjz = (double)q[3 * j + 2];
      const bool col_ok = sc_finite3(sjx, sjy, sjz) && sc_finite3(qjx, qjy, qjz);
      const double ex = six - sjx, ey = siy - sjy, ez = siz - sjz;
      const double fx = qix - qjx, fy = qiy - qjy, fz = qiz - qjz;
      const double ls2 = fma(ez, ez, fma(ey, ey, ex * ex));
      const double lt2 = fma(fz, fz, fma(fy, fy, fx * fx));
      const double a = (ls2 + lt2) - tau2;
      const bool c = col_ok && ls2 > 0.0 && lt2 > 0.0 && (a < 0.0 || a * a < 4.0 * (ls2 * lt2));   // false for NaN
      w |= (unsigned long long)(c ? 1 : 0) << jj;
    }
    if (!row_ok) w = 0;
    if (i < pb.cap) {
      M[(int64_t)i * pb.W + J] = w;
      if (w) atomicAdd(&dg[i], __popcll(w));
    }
    if (J != wk.a) {   // the tile below the diagonal: c_ji = c_ij to the bit
      unsigned long long tw = 0;
#pragma unroll 8
      for (int jj = 0; jj < 64; ++jj) {
        const unsigned long long b = __ballot((w >> jj) & 1ull);
        if (lane == jj) tw = b;
      }
      const int j = J * 64 + lane;
      if (j < pb.cap) {
        M[(int64_t)j * pb.W + wk.a] = tw;
        if (tw) atomicAdd(&dg[j], __popcll(tw));
      }
    }
  }
}

// grid (row blocks): the rank of a row = the rows of the problem with a larger key (deg << 32 | ~row)
__global__ __launch_bounds__(SC_BLOCK) void k_sc2_rank(const ScWork* __restrict__ work, const ScProb* __restrict__ probs,
                                                       const int32_t* __restrict__ d_m, int n_seeds,
                                                       const int32_t* __restrict__ deg, int32_t* __restrict__ seeds) {
  __shared__ int32_t lds[SC_BLOCK];
  const ScWork wk = work[blockIdx.x];
  const ScProb pb = probs[wk.prob];
  const int m = sc_rows(d_m, wk.prob, pb.cap);
  if (wk.a >= m) return;   // the same for the whole workgroup
  const int tid = threadIdx.x;
  const int i = wk.a + tid;
  const int32_t* dg = deg + pb.off;
  const bool live = i < m;
  const unsigned long long key = live ? ((unsigned long long)(unsigned)dg[i] << 32) | (unsigned)~i : 0ull;
  int rank = 0;
  for (int base = 0; base < m; base += SC_BLOCK) {
    const int n = min(SC_BLOCK, m - base);
    __syncthreads();
    if (tid < n) lds[tid] = dg[base + tid];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const unsigned long long other = ((unsigned long long)(unsigned)lds[j] << 32) | (unsigned)~(base + j);
      rank += other > key ? 1 : 0;
    }
  }
  if (live && rank < sc_seeds(n_seeds, m)) seeds[pb.soff + rank] = i;   // the keys differ: every rank < S is met once
}

// grid (seed tiles, SC_BLOCK / 4): one wave per seed.  cons [seed slot][SC_SET] rows in ascending order, cons_n their
// number (0: the seed is invalid).
__global__ __launch_bounds__(SC_BLOCK) void k_sc2_score(const ScWork* __restrict__ work, const ScProb* __restrict__ probs,
                                                        const int32_t* __restrict__ d_m, int n_seeds, int K,
                                                        const unsigned long long* __restrict__ mat,
                                                        const int32_t* __restrict__ seeds, int32_t* __restrict__ cons,
                                                        int32_t* __restrict__ cons_n) {
  const ScWork wk = work[blockIdx.x];
  const ScProb pb = probs[wk.prob];
  const int m = sc_rows(d_m, wk.prob, pb.cap);
  const int lane = threadIdx.x & 63;
  const int r = __builtin_amdgcn_readfirstlane(wk.a + (int)blockIdx.y * (SC_BLOCK / 64) + (int)(threadIdx.x >> 6));
  if (r >= wk.b || r >= sc_seeds(n_seeds, m)) return;   // the same for the whole wave; no barrier below
  const int sd = __builtin_amdgcn_readfirstlane(seeds[pb.soff + r]);
  const int Wm = (m + 63) >> 6;
  const unsigned long long* M = mat + pb.mat;
  const unsigned long long* row_s = M + (int64_t)sd * pb.W;
  unsigned long long rs[SC_ROW_REGS];
#pragma unroll
  for (int t = 0; t < SC_ROW_REGS; ++t) rs[t] = (lane + 64 * t < Wm) ? row_s[lane + 64 * t] : 0ull;
  unsigned long long top = 0;   // lane l: the key of rank l among those seen (0: none)
  int n_deg = 0;
  for (int w = 0; w < Wm; ++w) {
    unsigned long long bits = sc_uniform(row_s[w]);
    while (bits) {
      const int j = w * 64 + __builtin_ctzll(bits);
      bits &= bits - 1;
      const unsigned long long* row_j = M + (int64_t)j * pb.W;
      int c = 0;
#pragma unroll
      for (int t = 0; t < SC_ROW_REGS; ++t)
        if (64 * t < Wm) c += (lane + 64 * t < Wm) ? __popcll(rs[t] & row_j[lane + 64 * t]) : 0;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o);
      const unsigned long long key = ((unsigned long long)(unsigned)c << 32) | (unsigned)~j;   // never 0: ~j has bit 31
      const unsigned long long up = __shfl_up(top, 1);
      if (top < key) top = (lane == 0 || up > key) ? key : up;
      ++n_deg;
    }
  }
  const int n_take = min(K, n_deg);
  const int64_t slot = pb.soff + r;
  if (n_take + 1 < 3) {
    if (lane == 0) cons_n[slot] = 0;
    return;
  }
  // ascending row index: the position of a member = the members below it
  const bool mine = lane < n_take;
  const int jl = mine ? (int)~(unsigned)(top & 0xffffffffull) : 0x7fffffff;
  int pos = mine && sd < jl ? 1 : 0, pos_s = 0;
  for (int l = 0; l < n_take; ++l) {
    const int other = __shfl(jl, l);
    pos += other < jl ? 1 : 0;
    pos_s += other < sd ? 1 : 0;
  }
  if (mine) cons[slot * SC_SET + pos] = jl;
  if (lane == 0) {
    cons[slot * SC_SET + pos_s] = sd;
    cons_n[slot] = n_take + 1;
  }
}

// The fit of cs_ransac_fm_batch over the n >= 3 rows idx[0 .. n) of a problem (src, tgt: its first rows), in that order.
// true = valid, R = R | t.
__device__ bool sc_fit(const float* __restrict__ src, const float* __restrict__ tgt, const int32_t* __restrict__ idx, int n,
                       double (&R)[12]) {
  double cs_[3] = {0, 0, 0}, ct_[3] = {0, 0, 0};
  for (int k = 0; k < n; ++k) {
    const int64_t i = idx[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      cs_[c] += (double)src[3 * i + c];
      ct_[c] += (double)tgt[3 * i + c];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    cs_[c] = cs_[c] / (double)n;
    ct_[c] = ct_[c] / (double)n;
  }
  double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (int k = 0; k < n; ++k) {
    const int64_t i = idx[k];
    const double ds[3] = {(double)src[3 * i] - cs_[0], (double)src[3 * i + 1] - cs_[1], (double)src[3 * i + 2] - cs_[2]};
    const double dt[3] = {(double)tgt[3 * i] - ct_[0], (double)tgt[3 * i + 1] - ct_[1], (double)tgt[3 * i + 2] - ct_[2]};
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
  if (!horn_qcp(S, N, qv)) return false;   // no Jacobi here: a fit the solver declines is an invalid seed
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
  return ok;
}

// grid (seed tiles): one thread per seed.  hyp [seed slot][12], valid and cnt [seed slot].
__global__ __launch_bounds__(SC_BLOCK) void k_sc2_fit(const ScWork* __restrict__ work, const ScProb* __restrict__ probs,
                                                      const float* __restrict__ src, const float* __restrict__ tgt,
                                                      const int32_t* __restrict__ d_m, int n_seeds,
                                                      const int32_t* __restrict__ cons, const int32_t* __restrict__ cons_n,
                                                      double* __restrict__ hyp, int32_t* __restrict__ valid,
                                                      unsigned* __restrict__ cnt, unsigned long long* __restrict__ acc) {
  const ScWork wk = work[blockIdx.x];
  const ScProb pb = probs[wk.prob];
  const int m = sc_rows(d_m, wk.prob, pb.cap);
  const int r = wk.a + threadIdx.x;
  if (r >= wk.b) return;
  const int64_t slot = pb.soff + r;
  cnt[slot] = 0;
  bool ok = false;
  double R[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (r < sc_seeds(n_seeds, m)) {
    const int n = cons_n[slot];
    if (n >= 3) ok = sc_fit(src + 3 * pb.off, tgt + 3 * pb.off, cons + slot * SC_SET, n, R);
  }
  valid[slot] = ok ? 1 : 0;
  if (ok) {
#pragma unroll
    for (int e = 0; e < 12; ++e) hyp[slot * 12 + e] = R[e];
    atomicAdd(&acc[SC_ACC * (int64_t)wk.prob + SC_NVALID], 1ull);
  }
}

// grid (slices, seed tiles of the widest problem of the chunk)
__global__ __launch_bounds__(SC_BLOCK) void k_sc2_count(const ScWork* __restrict__ work, const ScProb* __restrict__ probs,
                                                        const float* __restrict__ src, const float* __restrict__ tgt,
                                                        const int32_t* __restrict__ d_m, int n_seeds, double thr2,
                                                        const double* __restrict__ hyp, const int32_t* __restrict__ valid,
                                                        unsigned* __restrict__ cnt) {
  __shared__ double lds[SC_TT][6];
  const ScWork wk = work[blockIdx.x];
  const ScProb pb = probs[wk.prob];
  const int m = sc_rows(d_m, wk.prob, pb.cap);
  const int S = sc_seeds(n_seeds, m);
  const int tid = threadIdx.x;
  const int r = blockIdx.y * SC_BLOCK + tid;
  const int r1 = min(wk.b, m);
  if (wk.a >= r1 || (int)blockIdx.y * SC_BLOCK >= S) return;   // the same for the whole workgroup
  const bool active = r < S && valid[pb.soff + r] != 0;
  double R[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) R[e] = active ? hyp[(pb.soff + r) * 12 + e] : 0.0;
  const float* s = src + 3 * pb.off;
  const float* q = tgt + 3 * pb.off;
  int c = 0;
  for (int base = wk.a; base < r1; base += SC_TT) {
    const int n = min(SC_TT, r1 - base);
    __syncthreads();
    for (int i = tid; i < n * 3; i += SC_BLOCK) {
      const int row = i / 3, col = i - 3 * row;
      lds[row][col] = (double)s[(int64_t)base * 3 + i];
      lds[row][3 + col] = (double)q[(int64_t)base * 3 + i];
    }
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < n; ++j) {
      const double* x = lds[j];
      c += sc_residual2(R, x[0], x[1], x[2], x[3], x[4], x[5]) < thr2 ? 1 : 0;   // false for NaN
    }
  }
  if (active && c) atomicAdd(&cnt[pb.soff + r], (unsigned)c);
}

// grid (seed tiles)
__global__ __launch_bounds__(SC_BLOCK) void k_sc2_best(const ScWork* __restrict__ work, const ScProb* __restrict__ probs,
                                                       const int32_t* __restrict__ valid, const unsigned* __restrict__ cnt,
                                                       unsigned long long* __restrict__ acc) {
  const ScWork wk = work[blockIdx.x];
  const ScProb pb = probs[wk.prob];
  const int r = wk.a + threadIdx.x;
  unsigned long long key = 0;
  if (r < wk.b && valid[pb.soff + r]) key = ((unsigned long long)cnt[pb.soff + r] << 32) | (unsigned)~r;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o);
    key = other > key ? other : key;
  }
  if ((threadIdx.x & 63) == 0 && (key >> 32)) atomicMax(&acc[SC_ACC * (int64_t)wk.prob + SC_BEST], key);
}

// One thread per problem: the winner and d_T.
__global__ void k_sc2_pick(const unsigned long long* __restrict__ acc, const ScProb* __restrict__ probs,
                           const int32_t* __restrict__ d_m, int n_prob, const int32_t* __restrict__ seeds,
                           const int32_t* __restrict__ deg, const double* __restrict__ hyp, ScSeg* __restrict__ segs,
                           double* __restrict__ d_T) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  const ScProb pb = probs[p];
  const unsigned long long key = acc[SC_ACC * (int64_t)p + SC_BEST];
  ScSeg sg = {};
  sg.m = sc_rows(d_m, p, pb.cap);
  sg.count = (int32_t)(key >> 32);
  sg.found = sg.m >= 3 && sg.count >= 3;
  if (sg.found) {
    sg.rank = (int32_t)(~(unsigned)(key & 0xffffffffull));
    sg.row = seeds[pb.soff + sg.rank];
    sg.deg = deg[pb.off + sg.row];
#pragma unroll
    for (int e = 0; e < 12; ++e) sg.R[e] = hyp[(pb.soff + sg.rank) * 12 + e];
  } else {
    sg.count = 0;
    sg.rank = sg.row = -1;
    sg.deg = 0;
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

// k = 61 - eM - ex with m <= 2^eM and thr2 = f 2^ex (ex from the host, clamped there): cs_ransac_fm_batch's rule
__device__ __forceinline__ int sc_shift(int m, int ex) {
  const int eM = m <= 1 ? 0 : 32 - __clz(m - 1);
  return 61 - eM - ex;
}

// grid (row blocks): the fixed-point squared error of the winner over its inliers, and the mask over every slot
__global__ __launch_bounds__(SC_BLOCK) void k_sc2_err(const ScWork* __restrict__ work, const ScProb* __restrict__ probs,
                                                      const float* __restrict__ src, const float* __restrict__ tgt,
                                                      const ScSeg* __restrict__ segs, double thr2, int ex,
                                                      unsigned long long* __restrict__ acc, uint8_t* __restrict__ d_inlier) {
  __shared__ unsigned long long part[SC_BLOCK / 64];
  const ScWork wk = work[blockIdx.x];
  const ScProb pb = probs[wk.prob];
  const ScSeg* sg = segs + wk.prob;
  const int row = wk.a + threadIdx.x;
  unsigned long long err = 0;
  bool inl = false;
  if (sg->found && row < wk.b && row < sg->m) {
    double R[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) R[e] = sg->R[e];
    const float* s = src + 3 * (pb.off + row);
    const float* q = tgt + 3 * (pb.off + row);
    const double d2 = sc_residual2(R, (double)s[0], (double)s[1], (double)s[2], (double)q[0], (double)q[1], (double)q[2]);
    if (d2 < thr2) {
      inl = true;
      err = (unsigned long long)(d2 * ldexp(1.0, sc_shift(sg->m, ex)));   // below 2^(61 - eM)
    }
  }
  if (d_inlier && row < wk.b) d_inlier[pb.off + row] = inl ? 1 : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) err += __shfl_xor(err, o);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = err;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long w = 0;
#pragma unroll
    for (int k = 0; k < SC_BLOCK / 64; ++k) w += part[k];
    if (w) atomicAdd(&acc[SC_ACC * (int64_t)wk.prob + SC_ERR], w);
  }
}

// One thread per problem: d_stat and d_rmse.
__global__ void k_sc2_out(const unsigned long long* __restrict__ acc, const ScSeg* __restrict__ segs, int n_prob, int ex,
                          int32_t* __restrict__ d_stat, double* __restrict__ d_rmse) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  const ScSeg* sg = segs + p;
  int32_t* st = d_stat + 6 * (int64_t)p;
  st[0] = sg->found;
  st[1] = sg->row;
  st[2] = sg->count;
  st[3] = (int32_t)acc[SC_ACC * (int64_t)p + SC_NVALID];
  st[4] = sg->rank;
  st[5] = sg->deg;
  double rmse = 0.0;
  if (sg->found) {
    const unsigned long long err = acc[SC_ACC * (int64_t)p + SC_ERR];
    rmse = sqrt(((double)err * ldexp(1.0, -sc_shift(sg->m, ex))) / (double)sg->count);
  }
  d_rmse[p] = rmse;
}

// a positive value of an environment variable (read per call), else the default
int64_t sc_env(const char* name, int64_t dflt) {
  const char* e = getenv(name);
  if (!e || !e[0]) return dflt;
  const long v = strtol(e, nullptr, 10);
  return v >= 1 && v < (1L << 31) ? (int64_t)v : dflt;
}

void sc_push(std::vector<ScWork>& work, int prob, int64_t n, int64_t step) {
  for (int64_t r = 0; r < n; r += step)
    work.push_back(ScWork{(int32_t)prob, (int32_t)r, (int32_t)std::min(n, r + step), 0});
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_sc2_batch(const float* d_src, const float* d_tgt, const int64_t* h_off, const int32_t* d_m, int n_prob,
                 double compat_dist, double max_corr, int n_seeds, int k_consensus, double* d_T, int32_t* d_stat,
                 double* d_rmse, uint8_t* d_inlier, void* stream) {
  const char* who = "cs_sc2_batch";
  char msg[256];
  const int bad = sc2_check_args(d_src, d_tgt, h_off, n_prob, compat_dist, max_corr, n_seeds, k_consensus, d_T, d_stat, d_rmse,
                                 msg, sizeof msg);
  CS_REQUIRE(bad == SC2_OK, bad, "%s", msg);
  if (n_prob == 0) return CS_OK;
  const double tau2 = compat_dist * compat_dist;   // +inf or 0 beyond 1.3e154 or below 1.5e-162
  const double thr2 = max_corr * max_corr;
  int ex = 1024;
  if (thr2 <= 1.7976931348623157e308) {
    frexp(thr2, &ex);
    ex = std::max(ex, -900);
  }
  const int64_t rows = h_off[n_prob] - h_off[0];
  const std::vector<std::pair<int, int>> chunks = sc2_plan(h_off, n_prob, sc2_chunk_bytes());
  const int64_t slice = sc_env("CS_SC2_SLICE", SC_SLICE), span = sc_env("CS_SC2_SPAN", SC_SPAN);
  // the problems, and per chunk the work lists of its kernels (first[c] .. first[c + 1] of each list)
  std::vector<ScProb> probs((size_t)n_prob);
  std::vector<ScWork> build, rowblk, seedtile, slices;
  std::vector<size_t> f_build, f_row, f_seed, f_slice;
  std::vector<int> y_tiles;
  int64_t soff = 0, max_words = 0;
  for (const auto& ch : chunks) {
    f_build.push_back(build.size());
    f_row.push_back(rowblk.size());
    f_seed.push_back(seedtile.size());
    f_slice.push_back(slices.size());
    int64_t words = 0, widest = 0;
    for (int p = ch.first; p < ch.second; ++p) {
      const int64_t cap = h_off[p + 1] - h_off[p], W = sc2_words(cap);
      const int64_t scap = n_seeds == 0 ? cap : std::min<int64_t>(n_seeds, cap);
      probs[p] = ScProb{h_off[p], words, soff, (int32_t)cap, (int32_t)W};
      words += cap * W;
      soff += scap;
      widest = std::max(widest, scap);
      for (int64_t I = 0; I < W; ++I)
        for (int64_t J = I; J < W; J += span)
          build.push_back(ScWork{(int32_t)p, (int32_t)I, (int32_t)J, (int32_t)std::min(W, J + span)});
      sc_push(rowblk, p, cap, SC_BLOCK);
      sc_push(seedtile, p, scap, SC_BLOCK);
      sc_push(slices, p, cap, slice);
    }
    max_words = std::max(max_words, words);
    y_tiles.push_back((int)ceil_div(widest, SC_BLOCK));
  }
  f_build.push_back(build.size());
  f_row.push_back(rowblk.size());
  f_seed.push_back(seedtile.size());
  f_slice.push_back(slices.size());
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const size_t n_acc = (size_t)SC_ACC * n_prob, n_seed = (size_t)soff;
  PoolBuf<ScProb> d_probs;
  PoolBuf<ScWork> d_build, d_row, d_seed, d_slice;
  PoolBuf<unsigned long long> mat((size_t)max_words), acc(n_acc);
  PoolBuf<int32_t> deg((size_t)rows), seeds(n_seed), cons(n_seed * SC_SET), cons_n(n_seed), valid(n_seed);
  PoolBuf<unsigned> cnt(n_seed);
  PoolBuf<double> hyp(12 * n_seed);
  PoolBuf<ScSeg> segs((size_t)n_prob);
  CS_REQUIRE(mat.p && acc.p && deg.p && seeds.p && cons.p && cons_n.p && valid.p && cnt.p && hyp.p && segs.p, CS_ERR_HIP,
             "%s: scratch allocation failed", who);
  int rc = upload(d_probs, probs, s);
  if (!rc && rows > 0) rc = upload(d_build, build, s);
  if (!rc && rows > 0) rc = upload(d_row, rowblk, s);
  if (!rc && rows > 0) rc = upload(d_seed, seedtile, s);
  if (!rc && rows > 0) rc = upload(d_slice, slices, s);
  if (rc) return rc;
  CS_HIP_CHECK(hipMemsetAsync(acc.p, 0, n_acc * sizeof(unsigned long long), s));
  if (rows > 0) CS_HIP_CHECK(hipMemsetAsync(deg.p, 0, (size_t)rows * sizeof(int32_t), s));
  if (d_inlier && h_off[0] > 0) CS_HIP_CHECK(hipMemsetAsync(d_inlier, 0, (size_t)h_off[0], s));
  // the scratch tables are indexed from the first slot of the call
  int32_t* deg0 = deg.p - h_off[0];
  double units = 0.0;
  for (int p = 0; p < n_prob; ++p) units += 17.0 * (double)(h_off[p + 1] - h_off[p]) * (double)(h_off[p + 1] - h_off[p]);
  ProfScope prof("sc2", s, units);
  const dim3 block(SC_BLOCK), g_prob((unsigned)ceil_div(n_prob, 256));
  for (size_t c = 0; c < chunks.size() && rows > 0; ++c) {
    const unsigned nb = (unsigned)(f_build[c + 1] - f_build[c]), nr = (unsigned)(f_row[c + 1] - f_row[c]),
                   ns = (unsigned)(f_seed[c + 1] - f_seed[c]), nl = (unsigned)(f_slice[c + 1] - f_slice[c]);
    if (nb == 0) continue;   // a chunk of empty problems
    hipLaunchKernelGGL(k_sc2_build, dim3(nb), dim3(64), 0, s, (const ScWork*)d_build.p + f_build[c], (const ScProb*)d_probs.p,
                       d_src, d_tgt, d_m, tau2, mat.p, deg0);
    hipLaunchKernelGGL(k_sc2_rank, dim3(nr), block, 0, s, (const ScWork*)d_row.p + f_row[c], (const ScProb*)d_probs.p, d_m,
                       n_seeds, (const int32_t*)deg0, seeds.p);
    hipLaunchKernelGGL(k_sc2_score, dim3(ns, SC_BLOCK / 4), block, 0, s, (const ScWork*)d_seed.p + f_seed[c],
                       (const ScProb*)d_probs.p, d_m, n_seeds, k_consensus, (const unsigned long long*)mat.p,
                       (const int32_t*)seeds.p, cons.p, cons_n.p);
    hipLaunchKernelGGL(k_sc2_fit, dim3(ns), block, 0, s, (const ScWork*)d_seed.p + f_seed[c], (const ScProb*)d_probs.p, d_src,
                       d_tgt, d_m, n_seeds, (const int32_t*)cons.p, (const int32_t*)cons_n.p, hyp.p, valid.p, cnt.p, acc.p);
    hipLaunchKernelGGL(k_sc2_count, dim3(nl, (unsigned)y_tiles[c]), block, 0, s, (const ScWork*)d_slice.p + f_slice[c],
                       (const ScProb*)d_probs.p, d_src, d_tgt, d_m, n_seeds, thr2, (const double*)hyp.p,
                       (const int32_t*)valid.p, cnt.p);
    hipLaunchKernelGGL(k_sc2_best, dim3(ns), block, 0, s, (const ScWork*)d_seed.p + f_seed[c], (const ScProb*)d_probs.p,
                       (const int32_t*)valid.p, (const unsigned*)cnt.p, acc.p);
  }
  hipLaunchKernelGGL(k_sc2_pick, g_prob, dim3(256), 0, s, (const unsigned long long*)acc.p, (const ScProb*)d_probs.p, d_m,
                     n_prob, (const int32_t*)seeds.p, (const int32_t*)deg0, (const double*)hyp.p, segs.p, d_T);
  if (rows > 0)
    hipLaunchKernelGGL(k_sc2_err, dim3((unsigned)rowblk.size()), block, 0, s, (const ScWork*)d_row.p, (const ScProb*)d_probs.p,
                       d_src, d_tgt, (const ScSeg*)segs.p, thr2, ex, acc.p, d_inlier);
  hipLaunchKernelGGL(k_sc2_out, g_prob, dim3(256), 0, s, (const unsigned long long*)acc.p, (const ScSeg*)segs.p, n_prob, ex,
                     d_stat, d_rmse);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // extern "C"
