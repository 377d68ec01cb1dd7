// Point-pair-feature voting: cs_ppf_batch, a fifth estimator beside cs_ransac_batch, cs_fgr_batch,
// cs_ransac_fm_batch and cs_sc2_batch, and the only one that reads no descriptor correspondences.  The specification is the
// comment of the call in include/corsair_hip.h; tests/ppf_ref.py restates it bit for bit.  The argument checks, the
// accumulator rule and the chunk planner stand in ppf_plan.h (plain C++); the constants of the bins in ppf_bounds.h.
//
// Once per call:
//   k_ppf_frame   one lane per row of every segment the call uses: the widened row, its unit normal and its local frame.
// Per chunk of whole problems (their tables and slabs fit CS_PPF_CHUNK_BYTES):
//   k_ppf_table   <0> counts and <1> fills the table of every (model, dist_step) of the chunk: one wave per (64 rows i, 64
//                 rows j), a lane owns i and walks the wave-uniform j.  Between them one exclusive sum (hipcub) over the
//                 counts of the chunk.  The slot of an entry inside its bucket comes from an integer atomic; every reader of
//                 a bucket adds integers, so that order reaches nothing.
//   k_ppf_vote    <1>: the accumulator (model rows x 30 u32) in the LDS, one workgroup per (problem, reference);
//                 <0>: in one of PPF_SLABS zeroed global slabs, a workgroup walks the items blockIdx.x, + gridDim.x, ...
//                 A lane owns scene rows i and walks the bucket of the pair (reference, i).  Then the peak: the u64 maximum
//                 of votes << 32 | ~cell (the slab path reads a cell and zeroes it in one atomic exchange).
// Once per call, behind the chunks:
//   k_ppf_rank    the rank of every reference by counting larger keys; the ranks < n_cand are the candidates.
//   k_ppf_pose    one lane per candidate: its pose.
//   k_ppf_verify  256 scene rows x one candidate per workgroup, the model rows staged through the LDS: the nearest model row
//                 of every posed scene row, the count and the fixed-point squared error by integer atomics.
//   k_ppf_out     one lane per problem: the winner, the inverse, every output row.
// Integer atomics only; no thread waits for another; every loop is bounded by an argument or by a segment's rows.  The
// shapes are first choices and not tuned.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "nn_common.h"
#include "ppf_bounds.h"
#include "ppf_plan.h"

namespace cs {
namespace {

static_assert(PPF_OK == CS_OK && PPF_INVALID == CS_ERR_INVALID && PPF_UNSUPPORTED == CS_ERR_UNSUPPORTED,
              "ppf_plan.h restates the codes of corsair_hip.h");

constexpr int PF_BLOCK = 256;        // lanes per workgroup of the row kernels
constexpr int PF_VOTE = 512;         // lanes per workgroup of the voting kernel
constexpr int PF_TT = 256;           // model rows per LDS stage of the verification (6 144 B as f64)
constexpr int PF_FR = 16;            // doubles per frame
constexpr int PF_LDS_HEAD = 16 + 8 * PF_FR + 8 * 14 + 8 * 28;   // bytes in front of the LDS accumulator: the u64 of the peak,
                                                             // the reference's frame, copies of the 14 cosines and of the
                                                             // 14 upper alpha boundaries
constexpr int PF_LDS_MAX = PF_LDS_HEAD + 4 * PPF_ALPHA_BINS * PPF_LDS_ROWS;
static_assert(PF_LDS_MAX <= 160 * 1024, "the accumulator of PPF_LDS_ROWS model rows fits the LDS of a CU");

// a frame: x (0..2), the unit normal u (3..5), the rows of the rotation that takes u to +x (6..14), ok (15)
enum { FX = 0, FU = 3, FR0 = 6, FR1 = 9, FR2 = 12, FOK = 15 };

__device__ const double PF_COS[14] = {CS_PPF_COS};
__device__ const double PF_BOUND[29][2] = {CS_PPF_ALPHA_BOUNDS};
__device__ const double PF_CENTRE[30][2] = {CS_PPF_ALPHA_CENTRES};

struct PfSeg {
  int64_t src;     // first row of the segment in its array
  int64_t fr;      // its first frame
  int32_t n, which;   // rows; 0 = scene array, 1 = model array
};

struct PfTab {
  int64_t mfr;     // first frame of the model
  int64_t keys;    // first counter of the table in the chunk's count and start arrays ((PPF_KEYS + 1) per table)
  int32_t m, pad;
  double step;
};

struct PfProb {
  int64_t sfr, mfr;   // first frames of the scene and of the model
  int64_t ref0;       // first peak slot of the problem
  int32_t ns, m, n_ref, tab;
};

struct PfWork {
  int32_t id, a, b, c;
};

struct PfEntry {
  int32_t row;
  float y, z;
};

__device__ __forceinline__ bool pf_finite(double v) { return fabs(v) < INFINITY; }   // false for NaN

__device__ void pf_frame(const float* __restrict__ x, const float* __restrict__ n, double* __restrict__ f) {
  const double X0 = (double)x[0], X1 = (double)x[1], X2 = (double)x[2];
  const double N0 = (double)n[0], N1 = (double)n[1], N2 = (double)n[2];
  const double nn = sqrt((N0 * N0 + N1 * N1) + N2 * N2);
  const bool ok = pf_finite(X0) && pf_finite(X1) && pf_finite(X2) && pf_finite(N0) && pf_finite(N1) && pf_finite(N2) && nn > 0.0;
  f[FX] = X0, f[FX + 1] = X1, f[FX + 2] = X2;
  double u0 = 0.0, u1 = 0.0, u2 = 0.0;
  if (ok) u0 = N0 / nn, u1 = N1 / nn, u2 = N2 / nn;
  f[FU] = u0, f[FU + 1] = u1, f[FU + 2] = u2;
  const double k = 1.0 + u0;
  if (ok && k >= 0x1.0p-20) {
    const double yz = (u1 * u2) / k;
    f[FR0] = u0, f[FR0 + 1] = u1, f[FR0 + 2] = u2;
    f[FR1] = -u1, f[FR1 + 1] = 1.0 - (u1 * u1) / k, f[FR1 + 2] = -yz;
    f[FR2] = -u2, f[FR2 + 1] = -yz, f[FR2 + 2] = 1.0 - (u2 * u2) / k;
  } else {   // u within 1.4e-3 rad of -x: the half turn about y
    f[FR0] = -1.0, f[FR0 + 1] = 0.0, f[FR0 + 2] = 0.0;
    f[FR1] = 0.0, f[FR1 + 1] = 1.0, f[FR1 + 2] = 0.0;
    f[FR2] = 0.0, f[FR2 + 1] = 0.0, f[FR2 + 2] = -1.0;
  }
  f[FOK] = ok ? 1.0 : 0.0;
}

__device__ __forceinline__ int pf_angle_bin(double c, const double* __restrict__ cosv) {
  int b = 0;
#pragma unroll
  for (int k = 0; k < 14; ++k) b += c <= cosv[k] ? 1 : 0;
  return b;
}

// The feature of the ordered pair (i, j) of one segment from their frames: false = the pair is skipped.  cosv: PF_COS or a copy.
__device__ __forceinline__ bool pf_pair(const double* __restrict__ fi, const double* __restrict__ fj, double step,
                                        const double* __restrict__ cosv, int& key, float& yf, float& zf) {
  if (fi[FOK] == 0.0 || fj[FOK] == 0.0) return false;
  const double dx = fj[FX] - fi[FX], dy = fj[FX + 1] - fi[FX + 1], dz = fj[FX + 2] - fi[FX + 2];
  const double len = sqrt((dx * dx + dy * dy) + dz * dz);
  if (!(len > 0.0)) return false;
  const double q = len / step;
  if (!(q < (double)PPF_DIST_BINS)) return false;
  const int dbin = (int)q;
  const double c1 = ((fi[FU] * dx + fi[FU + 1] * dy) + fi[FU + 2] * dz) / len;
  const double c2 = ((fj[FU] * dx + fj[FU + 1] * dy) + fj[FU + 2] * dz) / len;
  const double c3 = (fi[FU] * fj[FU] + fi[FU + 1] * fj[FU + 1]) + fi[FU + 2] * fj[FU + 2];
  yf = (float)((fi[FR1] * dx + fi[FR1 + 1] * dy) + fi[FR1 + 2] * dz);
  zf = (float)((fi[FR2] * dx + fi[FR2 + 1] * dy) + fi[FR2 + 2] * dz);
  if (!(fabsf(yf) < INFINITY && fabsf(zf) < INFINITY) || (yf == 0.0f && zf == 0.0f)) return false;
  key = ((dbin * PPF_ANGLE_BINS + pf_angle_bin(c1, cosv)) * PPF_ANGLE_BINS + pf_angle_bin(c2, cosv)) * PPF_ANGLE_BINS +
        pf_angle_bin(c3, cosv);
  return true;
}

// The bin of alpha = the angle of (ym + i zm) * conj(ys + i zs), in [-pi, pi): the boundaries not above it.  The table is
// mirrored to the bit -- boundary m of the lower half plane is (c, -s) of boundary 30 - m of the upper one
// (tools/gen_ppf_bounds.py asserts it) -- and c * py - (-s) * px = c * py + s * px = c * py - s * (-px) exactly, so the lower
// half plane counts over the upper half's 14 entries (bc, bs) with px negated: half the constants.
__device__ __forceinline__ int pf_alpha_bin(double ym, double zm, double ys, double zs, const double (&bc)[14],
                                            const double (&bs)[14]) {
  const double px = ym * ys + zm * zs, py = zm * ys - ym * zs;
  const bool lower = py < 0.0;
  const double qx = lower ? -px : px;
  int b = lower ? 0 : 15;
#pragma unroll
  for (int k = 0; k < 14; ++k) b += (bc[k] * py - bs[k] * qx) >= 0.0 ? 1 : 0;
  return b;
}

// grid (row tiles of the segments)
__global__ __launch_bounds__(PF_BLOCK) void k_ppf_frame(const PfWork* __restrict__ work, const PfSeg* __restrict__ segs,
                                                        const float* __restrict__ sx, const float* __restrict__ sn,
                                                        const float* __restrict__ mx, const float* __restrict__ mn,
                                                        double* __restrict__ frames) {
  const PfWork wk = work[blockIdx.x];
  const PfSeg sg = segs[wk.id];
  const int i = wk.a + threadIdx.x;
  if (i >= wk.b) return;
  const float* x = (sg.which ? mx : sx) + 3 * (sg.src + i);
  const float* n = (sg.which ? mn : sn) + 3 * (sg.src + i);
  pf_frame(x, n, frames + PF_FR * (sg.fr + i));
}

// grid (work items {table, i0, j0, j1}), one wave each.  FILL = 0: cnt[key] += 1;  FILL = 1: the entry goes to
// start[key] + (cnt[key] += 1) with cnt zeroed again by the host.
template <int FILL>
__global__ __launch_bounds__(64) void k_ppf_table(const PfWork* __restrict__ work, const PfTab* __restrict__ tabs,
                                                  const double* __restrict__ frames, int32_t* __restrict__ cnt,
                                                  const int32_t* __restrict__ start, PfEntry* __restrict__ ent) {
  const PfWork wk = work[blockIdx.x];
  const PfTab tb = tabs[wk.id];
  const int i = wk.a + threadIdx.x;
  if (i >= tb.m) return;   // no barrier below
  double fi[PF_FR];
  const double* F = frames + PF_FR * tb.mfr;
#pragma unroll
  for (int e = 0; e < PF_FR; ++e) fi[e] = F[PF_FR * (int64_t)i + e];
  for (int j = wk.b; j < wk.c; ++j) {
    int key;
    float y, z;
    if (j == i || !pf_pair(fi, F + PF_FR * (int64_t)j, tb.step, PF_COS, key, y, z)) continue;
    const int pos = atomicAdd(&cnt[tb.keys + key], 1);
    if (FILL) ent[(int64_t)start[tb.keys + key] + pos] = PfEntry{i, y, z};
  }
}

// items {problem, reference ordinal}.  LDS = 1: grid (items), dynamic LDS of PF_LDS_HEAD + 120 B x the largest model of the
// launch;  LDS = 0: grid (min(items, PPF_SLABS)), slab blockIdx.x of `slabs` (slab_cells u32 each, zero on entry and on exit).
template <int LDS>
__global__ __launch_bounds__(PF_VOTE) void k_ppf_vote(const PfWork* __restrict__ items, int n_items,
                                                      const PfProb* __restrict__ probs, const PfTab* __restrict__ tabs,
                                                      const double* __restrict__ frames, const int32_t* __restrict__ start,
                                                      const PfEntry* __restrict__ ent, int ref_step,
                                                      unsigned* __restrict__ slabs, int64_t slab_cells,
                                                      unsigned long long* __restrict__ peaks) {
  extern __shared__ __attribute__((aligned(16))) char pf_lds[];
  unsigned long long* s_best = reinterpret_cast<unsigned long long*>(pf_lds);
  double* fr = reinterpret_cast<double*>(pf_lds + 16);
  double* cosv = fr + PF_FR;
  double* bnd = cosv + 14;
  if (threadIdx.x < 14) cosv[threadIdx.x] = PF_COS[threadIdx.x];
  if (threadIdx.x < 28) bnd[threadIdx.x] = PF_BOUND[15 + (threadIdx.x >> 1)][threadIdx.x & 1];
  __syncthreads();
  // the 28 boundary constants in vector registers, through the LDS: as scalar constants they, the cosines, the reference's
  // frame and the arguments exceed the 102 scalar registers of a wave and spill
  double bc[14], bs[14];
#pragma unroll
  for (int k = 0; k < 14; ++k) bc[k] = bnd[2 * k], bs[k] = bnd[2 * k + 1];
  unsigned* acc = LDS ? reinterpret_cast<unsigned*>(pf_lds + PF_LDS_HEAD) : slabs + (int64_t)blockIdx.x * slab_cells;
  const int tid = threadIdx.x;
  for (int it = blockIdx.x; it < n_items; it += gridDim.x) {   // the same trips for the whole workgroup
    const PfWork wk = items[it];
    const PfProb pb = probs[wk.id];
    const PfTab tb = tabs[pb.tab];
    const int r = wk.a * ref_step;
    const int cells = pb.m * PPF_ALPHA_BINS;
    if (LDS)
      for (int c = tid; c < cells; c += PF_VOTE) acc[c] = 0u;
    if (tid == 0) *s_best = 0ull;
    // the reference's frame and the cosines are read from the LDS for the same reason
    const double* F = frames + PF_FR * pb.sfr;
    if (tid < PF_FR) fr[tid] = F[PF_FR * (int64_t)r + tid];
    __syncthreads();
    if (fr[FOK] != 0.0) {   // the same for the whole workgroup
      for (int i = tid; i < pb.ns; i += PF_VOTE) {
        int key;
        float ys, zs;
        if (i == r || !pf_pair(fr, F + PF_FR * (int64_t)i, tb.step, cosv, key, ys, zs)) continue;
        const int e0 = start[tb.keys + key], e1 = start[tb.keys + key + 1];
        for (int e = e0; e < e1; ++e) {
          const PfEntry en = ent[e];
          const int bin = pf_alpha_bin((double)en.y, (double)en.z, (double)ys, (double)zs, bc, bs);
          atomicAdd(&acc[en.row * PPF_ALPHA_BINS + bin], 1u);
        }
      }
    }
    __syncthreads();
    unsigned long long best = 0ull;
    for (int c = tid; c < cells; c += PF_VOTE) {
      // the slab path reads at the L2, where its atomics landed, and leaves the cell zero for the next item
      const unsigned v = LDS ? acc[c] : __hip_atomic_exchange(&acc[c], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v) {
        const unsigned long long key = ((unsigned long long)v << 32) | (unsigned)~c;
        best = key > best ? key : best;
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned long long other = __shfl_xor(best, o);
      best = other > best ? other : best;
    }
    if ((tid & 63) == 0 && best) atomicMax(s_best, best);
    __syncthreads();
    if (tid == 0) peaks[pb.ref0 + wk.a] = *s_best;
    __syncthreads();
  }
}

// grid (reference tiles {problem, a, b}): the rank of a reference = the references of the problem with a larger key
// (votes << 32 | ~ordinal); the ranks < n_cand are the candidates.
__global__ __launch_bounds__(PF_BLOCK) void k_ppf_rank(const PfWork* __restrict__ work, const PfProb* __restrict__ probs,
                                                       const unsigned long long* __restrict__ peaks, int n_cand,
                                                       int32_t* __restrict__ cand_ref) {
  __shared__ unsigned lds[PF_BLOCK];
  const PfWork wk = work[blockIdx.x];
  const PfProb pb = probs[wk.id];
  const int tid = threadIdx.x;
  const int k = wk.a + tid;
  const bool live = k < wk.b;
  const unsigned long long* pk = peaks + pb.ref0;
  const unsigned long long key = live ? ((pk[k] >> 32) << 32) | (unsigned)~k : 0ull;
  int rank = 0;
  for (int base = 0; base < pb.n_ref; base += PF_BLOCK) {
    const int n = min(PF_BLOCK, pb.n_ref - base);
    __syncthreads();
    if (tid < n) lds[tid] = (unsigned)(pk[base + tid] >> 32);
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const unsigned long long other = ((unsigned long long)lds[j] << 32) | (unsigned)~(base + j);
      rank += other > key ? 1 : 0;
    }
  }
  if (live && rank < n_cand) cand_ref[(int64_t)wk.id * PPF_MAX_CAND + rank] = k;   // the keys differ: every rank is met once
}

// One lane per (problem, candidate slot): hyp [slot][12] = R | t of Tm^-1 Rx(alpha) Ts, valid, and the zeroed sums.
__global__ __launch_bounds__(PF_BLOCK) void k_ppf_pose(const PfProb* __restrict__ probs, int n_prob, int n_cand, int ref_step,
                                                       const double* __restrict__ frames,
                                                       const unsigned long long* __restrict__ peaks,
                                                       const int32_t* __restrict__ cand_ref, double* __restrict__ hyp,
                                                       int32_t* __restrict__ valid, unsigned long long* __restrict__ sums) {
  const int t = blockIdx.x * PF_BLOCK + threadIdx.x;
  if (t >= n_prob * n_cand) return;
  const int p = t / n_cand, c = t - p * n_cand;
  const PfProb pb = probs[p];
  const int64_t slot = (int64_t)p * PPF_MAX_CAND + c;
  sums[2 * slot] = 0ull;
  sums[2 * slot + 1] = 0ull;
  int ok = 0;
  if (c < min(n_cand, pb.n_ref)) {
    const int k = cand_ref[slot];
    const unsigned long long peak = peaks[pb.ref0 + k];
    if (peak >> 32) {
      const int cell = (int)~(unsigned)(peak & 0xffffffffull);
      const int mr = cell / PPF_ALPHA_BINS, bin = cell - mr * PPF_ALPHA_BINS;
      const double* fs = frames + PF_FR * (pb.sfr + (int64_t)k * ref_step);
      const double* fm = frames + PF_FR * (pb.mfr + mr);
      const double ca = PF_CENTRE[bin][0], sa = PF_CENTRE[bin][1];
      double A[3][3], R[3][3];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        A[0][b] = fs[FR0 + b];
        A[1][b] = ca * fs[FR1 + b] - sa * fs[FR2 + b];
        A[2][b] = sa * fs[FR1 + b] + ca * fs[FR2 + b];
      }
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) R[a][b] = (fm[FR0 + a] * A[0][b] + fm[FR1 + a] * A[1][b]) + fm[FR2 + a] * A[2][b];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        hyp[slot * 12 + 4 * a] = R[a][0];
        hyp[slot * 12 + 4 * a + 1] = R[a][1];
        hyp[slot * 12 + 4 * a + 2] = R[a][2];
        hyp[slot * 12 + 4 * a + 3] = fm[FX + a] - ((R[a][0] * fs[FX] + R[a][1] * fs[FX + 1]) + R[a][2] * fs[FX + 2]);
      }
      ok = 1;
    }
  }
  valid[slot] = ok;
}

// k = 61 - eM - ex with ns <= 2^eM and thr2 = f 2^ex (ex from the host, clamped there): cs_sc2_batch's rule
__device__ __forceinline__ int pf_shift(int n, int ex) {
  const int eM = n <= 1 ? 0 : 32 - __clz(n - 1);
  return 61 - eM - ex;
}

// grid (scene tiles {problem, a, b}, n_cand): sums[slot] = {count, fixed-point squared error} of the candidate
__global__ __launch_bounds__(PF_BLOCK) void k_ppf_verify(const PfWork* __restrict__ work, const PfProb* __restrict__ probs,
                                                         const double* __restrict__ frames, const double* __restrict__ hyp,
                                                         const int32_t* __restrict__ valid, double thr2, int ex,
                                                         unsigned long long* __restrict__ sums) {
  __shared__ double lds[PF_TT][3];
  const PfWork wk = work[blockIdx.x];
  const PfProb pb = probs[wk.id];
  const int64_t slot = (int64_t)wk.id * PPF_MAX_CAND + blockIdx.y;
  if (!valid[slot]) return;   // the same for the whole workgroup
  const int tid = threadIdx.x;
  const int i = wk.a + tid;
  double T[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = hyp[slot * 12 + e];
  bool live = false;
  double px = 0, py = 0, pz = 0;
  if (i < wk.b) {
    const double* f = frames + PF_FR * (pb.sfr + i);
    const double x = f[FX], y = f[FX + 1], z = f[FX + 2];
    live = pf_finite(x) && pf_finite(y) && pf_finite(z);
    px = fma(T[2], z, fma(T[1], y, fma(T[0], x, T[3])));
    py = fma(T[6], z, fma(T[5], y, fma(T[4], x, T[7])));
    pz = fma(T[10], z, fma(T[9], y, fma(T[8], x, T[11])));
  }
  double dmin = INFINITY;
  const double* M = frames + PF_FR * pb.mfr;
  for (int base = 0; base < pb.m; base += PF_TT) {
    const int n = min(PF_TT, pb.m - base);
    __syncthreads();
    if (tid < n) {
      lds[tid][0] = M[PF_FR * (int64_t)(base + tid) + FX];
      lds[tid][1] = M[PF_FR * (int64_t)(base + tid) + FX + 1];
      lds[tid][2] = M[PF_FR * (int64_t)(base + tid) + FX + 2];
    }
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const double dx = px - lds[j][0], dy = py - lds[j][1], dz = pz - lds[j][2];
      const double d2 = fma(dz, dz, fma(dy, dy, dx * dx));
      dmin = d2 < dmin ? d2 : dmin;   // false for NaN
    }
  }
  unsigned long long cnt = 0, err = 0;
  if (live && dmin < thr2) {
    cnt = 1;
    err = (unsigned long long)(dmin * ldexp(1.0, pf_shift(pb.ns, ex)));   // below 2^(61 - eM)
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    cnt += __shfl_xor(cnt, o);
    err += __shfl_xor(err, o);
  }
  if ((tid & 63) == 0 && cnt) {
    atomicAdd(&sums[2 * slot], cnt);
    atomicAdd(&sums[2 * slot + 1], err);
  }
}

__device__ __forceinline__ void pf_identity(double* T) {
#pragma unroll
  for (int e = 0; e < 16; ++e) T[e] = (e % 5 == 0) ? 1.0 : 0.0;
}

// One lane per problem: every output row.
__global__ __launch_bounds__(PF_BLOCK) void k_ppf_out(const PfProb* __restrict__ probs, int n_prob, int n_cand, int ref_step,
                                                      int ex, const unsigned long long* __restrict__ peaks,
                                                      const int32_t* __restrict__ cand_ref, const double* __restrict__ hyp,
                                                      const int32_t* __restrict__ valid,
                                                      const unsigned long long* __restrict__ sums, double* __restrict__ d_T,
                                                      double* __restrict__ d_Tinv, int32_t* __restrict__ d_stat,
                                                      double* __restrict__ d_rmse, double* __restrict__ d_cand_T,
                                                      int32_t* __restrict__ d_cand_stat) {
  const int p = blockIdx.x * PF_BLOCK + threadIdx.x;
  if (p >= n_prob) return;
  const PfProb pb = probs[p];
  unsigned long long best = 0ull;
  for (int c = 0; c < n_cand; ++c) {
    const int64_t slot = (int64_t)p * PPF_MAX_CAND + c;
    double* T = d_cand_T + 16 * ((int64_t)p * n_cand + c);
    int32_t* st = d_cand_stat + 4 * ((int64_t)p * n_cand + c);
    if (valid[slot]) {
      const int k = cand_ref[slot];
      const unsigned long long peak = peaks[pb.ref0 + k];
#pragma unroll
      for (int e = 0; e < 12; ++e) T[e] = hyp[slot * 12 + e];
      T[12] = T[13] = T[14] = 0.0;
      T[15] = 1.0;
      st[0] = (int32_t)(peak >> 32);
      st[1] = (int32_t)sums[2 * slot];
      st[2] = k * ref_step;
      st[3] = (int32_t)~(unsigned)(peak & 0xffffffffull);
      const unsigned long long key = (sums[2 * slot] << 32) | (unsigned)~c;
      best = key > best ? key : best;
    } else {
      pf_identity(T);
      st[0] = st[1] = 0;
      st[2] = st[3] = -1;
    }
  }
  double* T = d_T + 16 * (int64_t)p;
  double* Ti = d_Tinv + 16 * (int64_t)p;
  int32_t* st = d_stat + 8 * (int64_t)p;
  st[7] = pb.n_ref;
  if (!best) {
    pf_identity(T);
    pf_identity(Ti);
    st[0] = st[1] = st[5] = 0;
    st[2] = st[3] = st[4] = st[6] = -1;
    d_rmse[p] = 0.0;
    return;
  }
  const int c = (int)~(unsigned)(best & 0xffffffffull);
  const int64_t slot = (int64_t)p * PPF_MAX_CAND + c;
  const int k = cand_ref[slot];
  const unsigned long long peak = peaks[pb.ref0 + k];
  const int cell = (int)~(unsigned)(peak & 0xffffffffull);
  const int count = (int)(best >> 32);
  double R[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) R[e] = T[e] = hyp[slot * 12 + e];
  T[12] = T[13] = T[14] = 0.0;
  T[15] = 1.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    Ti[4 * a] = R[a], Ti[4 * a + 1] = R[4 + a], Ti[4 * a + 2] = R[8 + a];
    Ti[4 * a + 3] = -((R[a] * R[3] + R[4 + a] * R[7]) + R[8 + a] * R[11]);
  }
  Ti[12] = Ti[13] = Ti[14] = 0.0;
  Ti[15] = 1.0;
  st[0] = 1;
  st[1] = (int32_t)(peak >> 32);
  st[2] = k * ref_step;
  st[3] = cell / PPF_ALPHA_BINS;
  st[4] = cell - st[3] * PPF_ALPHA_BINS;
  st[5] = count;
  st[6] = c;
  double rmse = 0.0;
  if (count > 0) rmse = sqrt(((double)sums[2 * slot + 1] * ldexp(1.0, -pf_shift(pb.ns, ex))) / (double)count);
  d_rmse[p] = rmse;
}

void pf_push(std::vector<PfWork>& work, int id, int64_t n, int64_t step) {
  for (int64_t r = 0; r < n; r += step) work.push_back(PfWork{(int32_t)id, (int32_t)r, (int32_t)std::min(n, r + step), 0});
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_ppf_batch(const float* d_scene, const float* d_scene_normal, const int64_t* h_soff, const float* d_model,
                 const float* d_model_normal, const int64_t* h_moff, const int32_t* h_scene_seg, const int32_t* h_model_seg,
                 int n_prob, const double* h_dist_step, double max_dist, int ref_step, int n_cand, double* d_T, double* d_Tinv,
                 int32_t* d_stat, double* d_rmse, double* d_cand_T, int32_t* d_cand_stat, void* stream) {
  const char* who = "cs_ppf_batch";
  char msg[320];
  const int bad = ppf_check_args(d_scene, d_scene_normal, h_soff, d_model, d_model_normal, h_moff, h_scene_seg, h_model_seg,
                                 n_prob, h_dist_step, max_dist, ref_step, n_cand, d_T, d_Tinv, d_stat, d_rmse, d_cand_T,
                                 d_cand_stat, msg, sizeof msg);
  CS_REQUIRE(bad == PPF_OK, bad, "%s", msg);
  if (n_prob == 0) return CS_OK;
  const double thr2 = max_dist * max_dist;
  int ex = 1024;
  if (thr2 <= 1.7976931348623157e308) {
    frexp(thr2, &ex);
    ex = std::max(ex, -900);
  }
  const int lds_rows = ppf_lds_rows();
  const std::vector<std::pair<int, int>> chunks = ppf_plan(h_moff, h_model_seg, n_prob, lds_rows, ppf_chunk_bytes());
  // the segments of the call, each framed once
  std::vector<PfSeg> segs;
  std::vector<PfWork> w_frame, w_ref, w_scene;
  std::map<std::pair<int, int>, int64_t> seg_fr;   // (which, segment id) -> first frame
  int64_t n_frames = 0;
  auto frame_of = [&](int which, int id, const int64_t* off) {
    const auto key = std::make_pair(which, id);
    const auto it = seg_fr.find(key);
    if (it != seg_fr.end()) return it->second;
    const int64_t n = off[id + 1] - off[id], at = n_frames;
    pf_push(w_frame, (int)segs.size(), n, PF_BLOCK);
    segs.push_back(PfSeg{off[id], at, (int32_t)n, which});
    seg_fr[key] = at;
    n_frames += n;
    return at;
  };
  std::vector<PfProb> probs((size_t)n_prob);
  std::vector<PfTab> tabs;
  // per chunk: its tables [t_first[c], t_first[c + 1]), the work of the table kernels and the items of the two voting launches
  std::vector<size_t> t_first, f_tab, f_lds, f_glb;
  std::vector<PfWork> w_tab, it_lds, it_glb;
  std::vector<int> lds_bytes;
  std::vector<int64_t> slab_cells, ent_total;
  int64_t n_refs = 0, max_ent = 0, max_tabs = 0, max_slab = 0;
  double units = 0.0;
  for (const auto& ch : chunks) {
    t_first.push_back(tabs.size());
    f_tab.push_back(w_tab.size());
    f_lds.push_back(it_lds.size());
    f_glb.push_back(it_glb.size());
    std::map<std::pair<int, uint64_t>, int> tab_of;   // (model segment, bits of dist_step) -> table of the chunk
    int64_t ent = 0, widest_lds = 0, widest_glb = 0;
    for (int p = ch.first; p < ch.second; ++p) {
      const int64_t ns = h_soff[h_scene_seg[p] + 1] - h_soff[h_scene_seg[p]];
      const int64_t m = h_moff[h_model_seg[p] + 1] - h_moff[h_model_seg[p]];
      const int64_t sfr = frame_of(0, h_scene_seg[p], h_soff), mfr = frame_of(1, h_model_seg[p], h_moff);
      uint64_t bits;
      memcpy(&bits, &h_dist_step[p], 8);
      const auto key = std::make_pair((int)h_model_seg[p], bits);
      auto it = tab_of.find(key);
      if (it == tab_of.end()) {
        const int t = (int)tabs.size();
        it = tab_of.emplace(key, t).first;
        tabs.push_back(PfTab{mfr, (int64_t)(t - (int)t_first.back()) * (PPF_KEYS + 1), (int32_t)m, 0, h_dist_step[p]});
        for (int64_t i0 = 0; i0 < m; i0 += 64)
          for (int64_t j0 = 0; j0 < m; j0 += 64)
            w_tab.push_back(PfWork{(int32_t)t, (int32_t)i0, (int32_t)j0, (int32_t)std::min(m, j0 + 64)});
        ent += m * m;
        units += 40.0 * (double)m * (double)m;
      }
      const int64_t n_ref = ns == 0 ? 0 : (ns - 1) / ref_step + 1;
      probs[p] = PfProb{sfr, mfr, n_refs, (int32_t)ns, (int32_t)m, (int32_t)n_ref, it->second};
      n_refs += n_ref;
      const bool in_lds = m <= lds_rows;
      if (ns > 0 && m > 0) {
        std::vector<PfWork>& items = in_lds ? it_lds : it_glb;
        for (int64_t k = 0; k < n_ref; ++k) items.push_back(PfWork{(int32_t)p, (int32_t)k, 0, 0});
        (in_lds ? widest_lds : widest_glb) = std::max(in_lds ? widest_lds : widest_glb, m);
      }
      pf_push(w_ref, p, n_ref, PF_BLOCK);
      if (m > 0) pf_push(w_scene, p, ns, PF_BLOCK);
      units += 40.0 * (double)n_ref * (double)ns + 11.0 * (double)n_cand * (double)ns * (double)m;
    }
    lds_bytes.push_back((int)(PF_LDS_HEAD + 4 * PPF_ALPHA_BINS * widest_lds));
    slab_cells.push_back(PPF_ALPHA_BINS * widest_glb);
    ent_total.push_back(ent);
    max_ent = std::max(max_ent, ent);
    max_tabs = std::max<int64_t>(max_tabs, (int64_t)(tabs.size() - t_first.back()));
    max_slab = std::max(max_slab, PPF_ALPHA_BINS * widest_glb);
  }
  t_first.push_back(tabs.size());
  f_tab.push_back(w_tab.size());
  f_lds.push_back(it_lds.size());
  f_glb.push_back(it_glb.size());
  CS_REQUIRE(max_ent < (1LL << 31), CS_ERR_UNSUPPORTED, "%s: the tables of one chunk exceed 2^31 entries: lower CS_PPF_CHUNK_BYTES",
             who);
  static const hipError_t vote_lds = hipFuncSetAttribute(reinterpret_cast<const void*>(k_ppf_vote<1>),
                                                         hipFuncAttributeMaxDynamicSharedMemorySize, PF_LDS_MAX);
  CS_HIP_CHECK(vote_lds);
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const size_t n_key = (size_t)max_tabs * (PPF_KEYS + 1), n_slot = (size_t)n_prob * PPF_MAX_CAND;
  PoolBuf<PfSeg> d_segs;
  PoolBuf<PfProb> d_probs;
  PoolBuf<PfTab> d_tabs;
  PoolBuf<PfWork> d_wframe, d_wref, d_wscene, d_wtab, d_lds, d_glb;
  PoolBuf<double> frames((size_t)n_frames * PF_FR), hyp(12 * n_slot);
  PoolBuf<int32_t> cnt(n_key), start(n_key), cand_ref(n_slot), valid(n_slot);
  PoolBuf<PfEntry> ent((size_t)max_ent);
  PoolBuf<unsigned> slabs((size_t)max_slab * PPF_SLABS);
  PoolBuf<unsigned long long> peaks((size_t)n_refs), sums(2 * n_slot);
  size_t tmp_bytes = 0;
  CS_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, cnt.p, start.p, (int)n_key, s));
  PoolBuf<char> tmp(tmp_bytes);
  CS_REQUIRE(frames.p && hyp.p && cnt.p && start.p && cand_ref.p && valid.p && ent.p && slabs.p && peaks.p && sums.p && tmp.p,
             CS_ERR_HIP, "%s: scratch allocation failed", who);
  int rc = upload(d_probs, probs, s);
  if (!rc) rc = upload(d_segs, segs, s);
  if (!rc) rc = upload(d_tabs, tabs, s);
  if (!rc) rc = upload(d_wframe, w_frame, s);
  if (!rc) rc = upload(d_wref, w_ref, s);
  if (!rc) rc = upload(d_wscene, w_scene, s);
  if (!rc) rc = upload(d_wtab, w_tab, s);
  if (!rc) rc = upload(d_lds, it_lds, s);
  if (!rc) rc = upload(d_glb, it_glb, s);
  if (rc) return rc;
  if (n_refs > 0) CS_HIP_CHECK(hipMemsetAsync(peaks.p, 0, (size_t)n_refs * sizeof(unsigned long long), s));
  if (max_slab > 0) CS_HIP_CHECK(hipMemsetAsync(slabs.p, 0, (size_t)max_slab * PPF_SLABS * sizeof(unsigned), s));
  ProfScope prof("ppf", s, units);
  const dim3 block(PF_BLOCK);
  if (!w_frame.empty())
    hipLaunchKernelGGL(k_ppf_frame, dim3((unsigned)w_frame.size()), block, 0, s, (const PfWork*)d_wframe.p, (const PfSeg*)d_segs.p,
                       d_scene, d_scene_normal, d_model, d_model_normal, frames.p);
  for (size_t c = 0; c < chunks.size(); ++c) {
    const unsigned nt = (unsigned)(f_tab[c + 1] - f_tab[c]), nl = (unsigned)(f_lds[c + 1] - f_lds[c]),
                   ng = (unsigned)(f_glb[c + 1] - f_glb[c]);
    if (nl + ng == 0) continue;   // no problem of the chunk has both a scene row and a model row
    const size_t keys = (t_first[c + 1] - t_first[c]) * (size_t)(PPF_KEYS + 1);
    const PfWork* wt = (const PfWork*)d_wtab.p + f_tab[c];
    CS_HIP_CHECK(hipMemsetAsync(cnt.p, 0, keys * sizeof(int32_t), s));
    if (nt) hipLaunchKernelGGL(k_ppf_table<0>, dim3(nt), dim3(64), 0, s, wt, (const PfTab*)d_tabs.p, (const double*)frames.p, cnt.p,
                               (const int32_t*)start.p, ent.p);
    CS_HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp_bytes, cnt.p, start.p, (int)keys, s));
    CS_HIP_CHECK(hipMemsetAsync(cnt.p, 0, keys * sizeof(int32_t), s));
    if (nt) hipLaunchKernelGGL(k_ppf_table<1>, dim3(nt), dim3(64), 0, s, wt, (const PfTab*)d_tabs.p, (const double*)frames.p, cnt.p,
                               (const int32_t*)start.p, ent.p);
    if (nl)
      hipLaunchKernelGGL(k_ppf_vote<1>, dim3(nl), dim3(PF_VOTE), (size_t)lds_bytes[c], s, (const PfWork*)d_lds.p + f_lds[c], (int)nl,
                         (const PfProb*)d_probs.p, (const PfTab*)d_tabs.p, (const double*)frames.p, (const int32_t*)start.p,
                         (const PfEntry*)ent.p, ref_step, (unsigned*)nullptr, (int64_t)0, peaks.p);
    if (ng)
      hipLaunchKernelGGL(k_ppf_vote<0>, dim3(std::min<unsigned>(ng, PPF_SLABS)), dim3(PF_VOTE), (size_t)PF_LDS_HEAD, s,
                         (const PfWork*)d_glb.p + f_glb[c], (int)ng, (const PfProb*)d_probs.p, (const PfTab*)d_tabs.p,
                         (const double*)frames.p, (const int32_t*)start.p, (const PfEntry*)ent.p, ref_step, slabs.p,
                         slab_cells[c], peaks.p);
  }
  if (!w_ref.empty())
    hipLaunchKernelGGL(k_ppf_rank, dim3((unsigned)w_ref.size()), block, 0, s, (const PfWork*)d_wref.p, (const PfProb*)d_probs.p,
                       (const unsigned long long*)peaks.p, n_cand, cand_ref.p);
  hipLaunchKernelGGL(k_ppf_pose, dim3((unsigned)ceil_div((int64_t)n_prob * n_cand, PF_BLOCK)), block, 0, s, (const PfProb*)d_probs.p,
                     n_prob, n_cand, ref_step, (const double*)frames.p, (const unsigned long long*)peaks.p,
                     (const int32_t*)cand_ref.p, hyp.p, valid.p, sums.p);
  if (!w_scene.empty())
    hipLaunchKernelGGL(k_ppf_verify, dim3((unsigned)w_scene.size(), (unsigned)n_cand), block, 0, s, (const PfWork*)d_wscene.p,
                       (const PfProb*)d_probs.p, (const double*)frames.p, (const double*)hyp.p, (const int32_t*)valid.p, thr2, ex,
                       sums.p);
  hipLaunchKernelGGL(k_ppf_out, dim3((unsigned)ceil_div(n_prob, PF_BLOCK)), block, 0, s, (const PfProb*)d_probs.p, n_prob, n_cand,
                     ref_step, ex, (const unsigned long long*)peaks.p, (const int32_t*)cand_ref.p, (const double*)hyp.p,
                     (const int32_t*)valid.p, (const unsigned long long*)sums.p, d_T, d_Tinv, d_stat, d_rmse, d_cand_T,
                     d_cand_stat);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // extern "C"
