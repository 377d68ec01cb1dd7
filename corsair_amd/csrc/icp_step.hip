// Set-up and step of the batched ICP.  k_icp_init: T from T0, the outputs cleared.  k_icp_frame:
// per problem the bounding box of its target segment (exact min / max), the origin and the power-of-two scales of its
// fixed-point sums (the derivation: icp_sums.h).  k_icp_step, one lane per problem and round: fitness / rmse of the
// association just made, the stop rule, Horn's fit (point) or the 6x6 / 7x7 normal equations by Cholesky (plane) from the
// sums, T <- U T.  The only ICP unit that includes the eigen-solvers (horn.h) and the small-pose update (icp_update.h).
#include <math.h>

#include "horn.h"
#include "icp.h"
#include "icp_update.h"

namespace cs {
namespace {

// eW: the exponent the plane scales give up to GICP's weight matrix (0 for every other estimation)
__global__ __launch_bounds__(256) void k_icp_frame(const IcpProb* __restrict__ probs, const float* __restrict__ tgt,
                                                   double max_dist, IcpFrame* __restrict__ frame,
                                                   IcpPlaneFrame* __restrict__ pframe, int eW) {
  __shared__ float red[2][3][4];
  const IcpProb pr = probs[blockIdx.x];
  const int tid = threadIdx.x;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t j = tid; j < pr.tn; j += 256) {
    const float* t = tgt + (pr.t0 + j) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      mn[c] = fminf(mn[c], t[c]);
      mx[c] = fmaxf(mx[c], t[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      mn[c] = fminf(mn[c], __shfl_xor(mn[c], off));
      mx[c] = fmaxf(mx[c], __shfl_xor(mx[c], off));
    }
    if ((tid & 63) == 0) {
      red[0][c][tid >> 6] = mn[c];
      red[1][c][tid >> 6] = mx[c];
    }
  }
  __syncthreads();
  if (tid != 0) return;
  IcpFrame f;
  double hmax = 0.0;
  bool finite = pr.tn > 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double lo = (double)fminf(fminf(red[0][c][0], red[0][c][1]), fminf(red[0][c][2], red[0][c][3]));
    const double hi = (double)fmaxf(fmaxf(red[1][c][0], red[1][c][1]), fmaxf(red[1][c][2], red[1][c][3]));
    f.o[c] = 0.5 * (lo + hi);
    const double h = 0.5 * (hi - lo);
    hmax = fmax(hmax, h);
    finite = finite && isfinite(f.o[c]) && isfinite(h);
  }
  if (!finite) {
    f.o[0] = f.o[1] = f.o[2] = 0.0;
    hmax = 0.0;
  }
  const double M = hmax + max_dist;
  int eM = 0;
  (void)frexp(M, &eM);                       // M = m 2^eM, 0.5 <= m < 1: M < 2^eM
  if (!isfinite(M)) eM = ICP_EM_MAX;
  eM = min(max(eM, ICP_EM_MIN), ICP_EM_MAX);
  const int eN = pr.sn <= 1 ? 0 : 32 - __clz(pr.sn - 1);   // n_src <= 2^eN
  const int s1 = ICP_SUM_BITS - eN - eM, s2 = ICP_SUM_BITS - eN - 2 * eM;
  f.sc1 = ldexp(1.0, s1);
  f.inv1 = ldexp(1.0, -s1);
  f.sc2 = ldexp(1.0, s2);
  f.inv2 = ldexp(1.0, -s2);
  f.clamp = ldexp(1.0, ICP_SUM_BITS - eN);
  f.sc_pp = ldexp(1.0, s2 - 2);
  f.inv_pp = ldexp(1.0, -(s2 - 2));
  frame[blockIdx.x] = f;
  if (pframe) {
    const int b = ICP_SUM_BITS - eN - eW;
    IcpPlaneFrame g;
    g.sc_rr = ldexp(1.0, b - 2 * eM - 3);
    g.inv_rr = ldexp(1.0, -(b - 2 * eM - 3));
    g.sc_rt = ldexp(1.0, b - eM - 2);
    g.inv_rt = ldexp(1.0, -(b - eM - 2));
    g.sc_tt = ldexp(1.0, b - 1);
    g.inv_tt = ldexp(1.0, -(b - 1));
    g.sc_rd = ldexp(1.0, b - 2 * eM - 2);
    g.inv_rd = ldexp(1.0, -(b - 2 * eM - 2));
    g.sc_td = ldexp(1.0, b - eM - 1);
    g.inv_td = ldexp(1.0, -(b - eM - 1));
    pframe[blockIdx.x] = g;
  }
}

__device__ __forceinline__ bool icp_all_finite(const double* v, int n) {
  bool f = true;
  for (int i = 0; i < n; ++i) f = f && isfinite(v[i]);
  return f;
}

// The scale step of EST = 3, 4: the problem stops (false) when s_u is not a finite positive number or the accumulated scale
// s_u * scale would leave [scale_min, scale_max] (a NaN fails both comparisons).
__device__ __forceinline__ bool icp_scale_ok(double su, double scale, const IcpCriteria& crit, double& scale_new) {
  scale_new = su * scale;
  return isfinite(su) && su > 0.0 && scale_new >= crit.scale_min && scale_new <= crit.scale_max;
}

// The point-to-point update from the 17 sums: Horn's fit about the means.  SCALE: Umeyama's scale from the 18th sum on top
// of it, U = [s_u R | q_mean - s_u R p_mean]; false = the problem stops on the scale rules.
template <bool SCALE>
__device__ __forceinline__ bool icp_update_point(const unsigned long long* __restrict__ S, double dn, const IcpFrame& fr,
                                                 const double* __restrict__ Tp, double (&Tn)[12], double scale,
                                                 const IcpCriteria& crit, double& scale_new) {
  double sp[3], sq[3], mp[3], mq[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sp[c] = (double)(long long)S[1 + c] * fr.inv1;
    sq[c] = (double)(long long)S[4 + c] * fr.inv1;
    mp[c] = sp[c] / dn;
    mq[c] = sq[c] / dn;
  }
  // cross-covariance about the means, source index first (the RANSAC's S): sum p'_a q'_b - (sum p'_a) mean q'_b
  double Sm[3][3], N[4][4], V[4][4];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) Sm[a][b] = fma(-sp[a], mq[b], (double)(long long)S[7 + 3 * a + b] * fr.inv2);
  N[0][0] = Sm[0][0] + Sm[1][1] + Sm[2][2];
  N[0][1] = Sm[1][2] - Sm[2][1];
  N[0][2] = Sm[2][0] - Sm[0][2];
  N[0][3] = Sm[0][1] - Sm[1][0];
  N[1][1] = Sm[0][0] - Sm[1][1] - Sm[2][2];
  N[1][2] = Sm[0][1] + Sm[1][0];
  N[1][3] = Sm[2][0] + Sm[0][2];
  N[2][2] = -Sm[0][0] + Sm[1][1] - Sm[2][2];
  N[2][3] = Sm[1][2] + Sm[2][1];
  N[3][3] = -Sm[0][0] - Sm[1][1] + Sm[2][2];
  N[1][0] = N[0][1];
  N[2][0] = N[0][2];
  N[3][0] = N[0][3];
  N[2][1] = N[1][2];
  N[3][1] = N[1][3];
  N[3][2] = N[2][3];
  double qv[4];
  if (!horn_qcp(Sm, N, qv)) {
    jacobi4(N, V);
    // eigenvector of the largest eigenvalue (ties -> lowest index), as the RANSAC selects it
    double best = N[0][0];
    qv[0] = V[0][0]; qv[1] = V[1][0]; qv[2] = V[2][0]; qv[3] = V[3][0];
#pragma unroll
    for (int c = 1; c < 4; ++c) {
      if (N[c][c] > best) {
        best = N[c][c];
        qv[0] = V[0][c];
        qv[1] = V[1][c];
        qv[2] = V[2][c];
        qv[3] = V[3][c];
      }
    }
  }
  double R[3][3];
  icp_quat_rotation(qv[0], qv[1], qv[2], qv[3], R);
  // t = q_mean - R p_mean on the unprimed means; T <- U T
  double pm[3], qm[3], t[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    pm[c] = mp[c] + fr.o[c];
    qm[c] = mq[c] + fr.o[c];
  }
  if constexpr (SCALE) {
    // s_u = sum_ab R_ab S_ab / (sum p'.p' - sum_a (sum p'_a) mean p'_a): the variance of the posed sources about their mean
    double den = (double)(long long)S[17] * fr.inv_pp;
#pragma unroll
    for (int a = 0; a < 3; ++a) den = fma(-sp[a], mp[a], den);
    double num = R[0][0] * Sm[0][0];
#pragma unroll
    for (int k = 1; k < 9; ++k) num = fma(R[k / 3][k % 3], Sm[k / 3][k % 3], num);
    if (!(isfinite(den) && den > 0.0)) return false;
    const double su = num / den;
    if (!icp_scale_ok(su, scale, crit, scale_new)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t[a] = fma(-su, fma(R[a][2], pm[2], fma(R[a][1], pm[1], R[a][0] * pm[0])), qm[a]);
#pragma unroll
      for (int b = 0; b < 3; ++b) R[a][b] = su * R[a][b];
    }
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) t[a] = qm[a] - fma(R[a][2], pm[2], fma(R[a][1], pm[1], R[a][0] * pm[0]));
  }
  icp_compose(R, t, Tp, Tn);
  return true;
}

// The point-to-plane update from the 29 sums (the weighted layout has the same entries in the same places): A x = -b by an
// unpivoted Cholesky, x = (alpha, t') about the origin o, the rotation of the quaternion (1, alpha / 2).  false: a pivot is
// not finite or too small -- the problem stops.  NJ = 7 (plane + scale): the 37 sums, a seventh unknown sigma,
// s_u = 1 + sigma, U = [s_u R | t' + o - s_u R o]; false also when the scale rules stop the problem.
template <int NJ>
__device__ __forceinline__ bool icp_update_plane(const unsigned long long* __restrict__ S, const IcpFrame& fr,
                                                 const IcpPlaneFrame& g, const double* __restrict__ Tp, double (&Tn)[12],
                                                 double scale, const IcpCriteria& crit, double& scale_new) {
  constexpr int NJJ = NJ * (NJ + 1) / 2;
  double A[NJ][NJ], bv[NJ], xv[NJ];
  {
    int at = 1;
#pragma unroll
    for (int i = 0; i < NJ; ++i)
#pragma unroll
      for (int j = i; j < NJ; ++j) {
        const bool ri = icp_rot_col(i), rj = icp_rot_col(j);
        const double inv = ri && rj ? g.inv_rr : (ri || rj ? g.inv_rt : g.inv_tt);
        A[i][j] = (double)(long long)S[at++] * inv;
        A[j][i] = A[i][j];
      }
  }
#pragma unroll
  for (int i = 0; i < NJ; ++i) bv[i] = (double)(long long)S[1 + NJJ + i] * (icp_rot_col(i) ? g.inv_rd : g.inv_td);
  if (!icp_chol_solve<NJ>(A, bv, xv)) return false;
  double R[3][3], t[3];
  icp_quat_rotation(1.0, 0.5 * xv[0], 0.5 * xv[1], 0.5 * xv[2], R);
  if constexpr (NJ == 7) {
    // p <- s_u R (p - o) + t' + o:  t = t' + o - s_u R o
    const double su = 1.0 + xv[6];
    if (!icp_scale_ok(su, scale, crit, scale_new)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      t[a] = fma(-su, fma(R[a][2], fr.o[2], fma(R[a][1], fr.o[1], R[a][0] * fr.o[0])), xv[3 + a] + fr.o[a]);
#pragma unroll
      for (int b = 0; b < 3; ++b) R[a][b] = su * R[a][b];
    }
  } else {
    // p <- R (p - o) + t' + o:  t = t' + o - R o
#pragma unroll
    for (int a = 0; a < 3; ++a)
      t[a] = (xv[3 + a] + fr.o[a]) - fma(R[a][2], fr.o[2], fma(R[a][1], fr.o[1], R[a][0] * fr.o[0]));
  }
  icp_compose(R, t, Tp, Tn);
  return true;
}

// One lane per problem: the evaluation of the association just made, the stop rule, the update.  last = the round after
// the max_iter-th update (or the only one when max_iter = 0): nothing is fitted, the f32 copy of T is written.
template <int EST>
__global__ void k_icp_step(const IcpProb* __restrict__ probs, int n_prob, const IcpFrame* __restrict__ frame,
                           const IcpPlaneFrame* __restrict__ pframe, IcpCriteria crit, int round, int last,
                           unsigned long long* __restrict__ sums, int32_t* __restrict__ done, double* __restrict__ T,
                           float* __restrict__ T32, double* __restrict__ fitness, double* __restrict__ rmse,
                           double* __restrict__ wfitness, double* __restrict__ scale, int32_t* __restrict__ iters,
                           int32_t* __restrict__ ncorr, double* __restrict__ mrmse) {
  constexpr int NS = icp_nsum(EST);
  constexpr int MIN_CORR = icp_is_plane(EST) ? icp_nj(EST) : 3;   // one pair per unknown of the plane system
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  double* Tp = T + (int64_t)p * 16;
  if (!done[p]) {
    const IcpProb pr = probs[p];
    const IcpFrame fr = frame[p];
    unsigned long long* S = sums + (int64_t)p * NS;
    const long long n = (long long)S[0];
    const double dn = (double)n;
    const double fit = pr.sn > 0 ? dn / (double)pr.sn : 0.0;
    const double sd2 = (double)(long long)S[icp_d2_at(EST)] * fr.inv2;
    const double rm = n > 0 ? sqrt(sd2 / dn) : 0.0;
    const double pfit = fitness[p], prm = rmse[p];
    fitness[p] = fit;
    rmse[p] = rm;
    ncorr[p] = (int32_t)n;
    if (wfitness) {   // sum w = S_w 2^-(61 - eN); every weight is 1 without a kernel, and the share is the fitness
      if constexpr (EST == ICP_ROBUST)
        wfitness[p] = pr.sn > 0 ? ((double)(long long)S[NS - 1] * (1.0 / fr.clamp)) / (double)pr.sn : 0.0;
      else
        wfitness[p] = fit;
    }
    if constexpr (EST == ICP_GICP) {   // the Mahalanobis rmse of this association: sum e.We shares the scale of rot x e
      if (mrmse) {
        const double sm = (double)(long long)S[NS - 1] * pframe[p].inv_rd;
        mrmse[p] = n > 0 && sm > 0.0 ? sqrt(sm / dn) : 0.0;
      }
    }
    bool stop = last != 0;
    if (round > 0 && fabs(fit - pfit) < crit.rel_fitness && fabs(rm - prm) < crit.rel_rmse) stop = true;
    if (n < MIN_CORR || !isfinite(fit) || !isfinite(rm)) stop = true;
    if (!stop) {
      double Tn[12];
      bool solved = true;
      double sc_old = 1.0, sc_new = 1.0;   // the accumulated scale before and after this update (EST = 3, 4)
      if constexpr (icp_has_scale(EST)) sc_old = scale[p];
      if constexpr (icp_is_plane(EST))
        solved = icp_update_plane<icp_nj(EST)>(S, fr, pframe[p], Tp, Tn, sc_old, crit, sc_new);
      else
        solved = icp_update_point<EST == ICP_POINT_S>(S, dn, fr, Tp, Tn, sc_old, crit, sc_new);
      if (solved && icp_all_finite(Tn, 12)) {
#pragma unroll
        for (int i = 0; i < 12; ++i) Tp[i] = Tn[i];
        if constexpr (icp_has_scale(EST)) scale[p] = sc_new;
        iters[p] = iters[p] + 1;
#pragma unroll
        for (int k = 0; k < NS; ++k) S[k] = 0;
      } else {
        stop = true;
      }
    }
    if (stop) done[p] = 1;
  }
  if (last && T32) {
    for (int i = 0; i < 16; ++i) T32[(int64_t)p * 16 + i] = (float)Tp[i];
  }
}

__global__ void k_icp_init(const float* __restrict__ T0, int n_prob, double* __restrict__ T, double* __restrict__ fitness,
                           double* __restrict__ rmse, double* __restrict__ wfitness, double* __restrict__ scale,
                           int32_t* __restrict__ iters, int32_t* __restrict__ ncorr, int32_t* __restrict__ done) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  for (int i = 0; i < 16; ++i) T[(int64_t)p * 16 + i] = (double)T0[(int64_t)p * 16 + i];
  fitness[p] = 0.0;
  rmse[p] = 0.0;
  if (wfitness) wfitness[p] = 0.0;
  if (scale) scale[p] = 1.0;
  iters[p] = 0;
  ncorr[p] = 0;
  done[p] = 0;
}

dim3 problem_grid(int n_prob) { return dim3((unsigned)ceil_div(n_prob, 64)); }   // one lane per problem

template <int EST>
void launch_step(const IcpCall& c, const IcpState& w, int round, int last, hipStream_t s) {
  hipLaunchKernelGGL(k_icp_step<EST>, problem_grid(c.n_prob), dim3(64), 0, s, w.probs, c.n_prob, w.frame, w.pframe, w.crit,
                     round, last, w.sums, w.done, c.T, c.T32, c.fitness, c.rmse, c.wfitness, c.scale, c.iters, c.ncorr,
                     c.mrmse);
}

}  // namespace

void icp_launch_setup(int est, const IcpCall& c, const IcpState& w, hipStream_t s) {
  hipLaunchKernelGGL(k_icp_init, problem_grid(c.n_prob), dim3(64), 0, s, c.T0, c.n_prob, c.T, c.fitness, c.rmse, c.wfitness,
                     icp_has_scale(est) ? c.scale : (double*)nullptr, c.iters, c.ncorr, w.done);
  hipLaunchKernelGGL(k_icp_frame, dim3((unsigned)c.n_prob), dim3(256), 0, s, w.probs, c.tgt, c.max_dist, w.frame, w.pframe,
                     w.eW);
}

void icp_launch_step(int est, const IcpCall& c, const IcpState& w, int round, int last, hipStream_t s) {
  switch (est) {
    case ICP_POINT: return launch_step<ICP_POINT>(c, w, round, last, s);
    case ICP_PLANE: return launch_step<ICP_PLANE>(c, w, round, last, s);
    case ICP_ROBUST: return launch_step<ICP_ROBUST>(c, w, round, last, s);
    case ICP_POINT_S: return launch_step<ICP_POINT_S>(c, w, round, last, s);
    case ICP_PLANE_S: return launch_step<ICP_PLANE_S>(c, w, round, last, s);
    case ICP_GICP: return launch_step<ICP_GICP>(c, w, round, last, s);
  }
}

}  // namespace cs
