// Batched ICP: point-to-point (cs_icp_batch), point-to-plane (cs_icp_plane_batch),
// point-to-plane with a robust kernel (cs_icp_plane_robust_batch), both estimations with an isotropic scale
// (cs_icp_scale_batch) and plane-to-plane, Generalized ICP (cs_icp_gicp_batch).  The specifications are the comments of the
// five entries in include/corsair_hip.h; tests/icp_ref.py, tests/icp_plane_ref.py, tests/icp_robust_ref.py,
// tests/icp_scale_ref.py and tests/gicp_ref.py restate them bit for bit.  This unit is the host side: the five entries check
// their own arguments, fill an IcpCall and name the estimation (icp.h); icp_run is the one driver.  Pose chain, association,
// evaluation, loop and stop rule are one code; the estimation selects the sums at the end of the association kernels
// (icp_sums.h, icp_assoc.hip) and the update (icp_step.hip).  The rigid estimations are what they were before the others
// existed: kernel = L2 runs EST = 1, nothing of EST = 3 / 4 is launched unless cs_icp_scale_batch is called and nothing of
// EST = 5 unless cs_icp_gicp_batch is.
//
// One call = one target preparation + (max_iter + 1) rounds, all enqueued without a host wait:
//   k_icp_frame    per problem: the bounding box of its target segment (exact min / max), the origin and the
//                  power-of-two scales of its fixed-point sums
//   ChfImage       the f16 hi / lo image, |S t|^2 and the float4 rows of every target (chf_rank.h), once per call
//   round r:       k_icp_f16 (+ k_icp_exact for the workgroups it flags) or k_icp_exact alone -- association of the posed
//                  ORIGINAL sources under the current T, 17 (point), 29 (plane), 30 (weighted plane), 18 (point + scale),
//                  37 (plane + scale) or 30 (GICP) order-free 64-bit integer sums per problem; k_icp_step -- one lane per problem:
//                  fitness / rmse of that association, the stop rule, Horn's fit (point) or the 6x6 / 7x7 normal equations
//                  by Cholesky (plane) from the sums, T <- U T.
// A problem that has stopped raises its device flag; its workgroups leave on it in every later round.
#include <math.h>

#include <algorithm>

#include "chf_rank.h"
#include "icp.h"

namespace cs {
namespace {

std::atomic<unsigned long long> g_icp_stats[2];

int icp_run(const char* name, int est, const IcpCall& c) {
  const int NS = icp_nsum(est), n_prob = c.n_prob;
  CS_REQUIRE(c.soff && c.toff && c.src_seg && c.tgt_seg, CS_ERR_INVALID, "%s: NULL table", name);
  CS_REQUIRE(n_prob >= 0, CS_ERR_INVALID, "%s: negative problem count", name);
  CS_REQUIRE(c.max_dist > 0.0 && std::isfinite(c.max_dist), CS_ERR_INVALID, "%s: max_dist must be positive and finite",
             name);
  CS_REQUIRE(c.max_iter >= 0 && c.max_iter <= 1000, CS_ERR_UNSUPPORTED, "%s: max_iter outside [0, 1000]", name);
  CS_REQUIRE(!std::isnan(c.relative_fitness) && !std::isnan(c.relative_rmse), CS_ERR_INVALID,
             "%s: a convergence threshold is NaN", name);
  if (n_prob == 0) return CS_OK;
  CS_REQUIRE(c.T0 && c.T && c.fitness && c.rmse && c.iters && c.ncorr, CS_ERR_INVALID, "%s: NULL argument", name);
  CS_REQUIRE(!icp_has_scale(est) || c.scale, CS_ERR_INVALID, "%s: NULL scale output", name);
  std::vector<IcpProb> probs(n_prob);
  std::vector<IcpWork> work;
  int64_t nt_rows = 0, n_corr_rows = 0;
  double flop = 0.0;
  for (int p = 0; p < n_prob; ++p) {
    const int ss = c.src_seg[p], ts = c.tgt_seg[p];
    CS_REQUIRE(ss >= 0 && ts >= 0, CS_ERR_INVALID, "%s: negative segment id in problem %d", name, p);
    const int64_t sn = c.soff[ss + 1] - c.soff[ss], tn = c.toff[ts + 1] - c.toff[ts];
    CS_REQUIRE(sn >= 0 && tn >= 0, CS_ERR_INVALID, "%s: bad segment in problem %d", name, p);
    CS_REQUIRE(sn < (1LL << 31) && tn < (1LL << 31), CS_ERR_UNSUPPORTED,
               "%s: a segment of problem %d has 2^31 rows or more", name, p);
    IcpProb& pr = probs[p];
    pr.s0 = c.soff[ss];
    pr.t0 = c.toff[ts];
    pr.c0 = n_corr_rows;
    pr.sn = (int32_t)sn;
    pr.tn = (int32_t)tn;
    if (tn > 0) nt_rows = std::max<int64_t>(nt_rows, c.toff[ts + 1]);
    for (int64_t q = 0; q < sn; q += ICP_ST) {
      IcpWork w;
      w.s0 = pr.s0 + q;
      w.c0 = pr.c0 + q;
      w.sn = (int32_t)std::min<int64_t>(sn - q, ICP_ST);
      w.prob = p;
      work.push_back(w);
    }
    n_corr_rows += sn;
    flop += 8.0 * (double)sn * (double)tn;
  }
  CS_REQUIRE(work.empty() || c.src, CS_ERR_INVALID, "%s: NULL source array", name);
  CS_REQUIRE(nt_rows == 0 || c.tgt, CS_ERR_INVALID, "%s: NULL target array", name);
  CS_REQUIRE(!icp_is_plane(est) || nt_rows == 0 || c.tnrm, CS_ERR_INVALID, "%s: NULL target normal array", name);
  CS_REQUIRE(est != ICP_GICP || work.empty() || c.snrm, CS_ERR_INVALID, "%s: NULL source normal array", name);
  IcpState st{};
  // GICP: 1 - eps, and eW = the smallest integer with 1 / (2 eps) <= 2^eW, i.e. 1 <= eps * 2^(eW + 1) (exact); in [-1, 9]
  st.ome = 1.0 - c.epsilon;
  if (est == ICP_GICP)
    for (st.eW = -1; std::ldexp(c.epsilon, st.eW + 1) < 1.0; ++st.eW) {
    }
  st.crit.thr2 = c.max_dist * c.max_dist;
  st.crit.rel_fitness = c.relative_fitness;
  st.crit.rel_rmse = c.relative_rmse;
  st.crit.scale_min = c.scale_min;
  st.crit.scale_max = c.scale_max;
  hipStream_t s = (hipStream_t)c.stream;
  pool_use_stream(s);
  const bool use_f16 = !env_first_is("CS_ICP_F16", '0');
  const bool want_stats = use_f16 && env_first_is("CS_ICP_STATS", '1');
  st.n_work = (unsigned)work.size();
  PoolBuf<IcpProb> dprob;
  PoolBuf<IcpWork> dwork;
  PoolBuf<IcpFrame> frame((size_t)n_prob);
  PoolBuf<IcpPlaneFrame> pframe;
  PoolBuf<unsigned long long> sums((size_t)n_prob * NS + 2);   // + the two statistics counters
  PoolBuf<int32_t> done((size_t)n_prob);
  CS_REQUIRE(frame.p && sums.p && done.p, CS_ERR_HIP, "%s: scratch allocation failed", name);
  if (icp_is_plane(est)) CS_REQUIRE(pframe.alloc((size_t)n_prob), CS_ERR_HIP, "%s: scratch allocation failed", name);
  int rc = upload(dprob, probs, s);
  if (!rc) rc = upload(dwork, work, s);
  if (rc) return rc;
  unsigned long long* dstats = sums.p + (size_t)n_prob * NS;
  st.probs = dprob.p;
  st.work = dwork.p;
  st.frame = frame.p;
  st.pframe = pframe.p;
  st.sums = sums.p;
  st.stats = want_stats ? dstats : nullptr;
  st.done = done.p;
  ProfScope prof("icp", s, flop * (double)(c.max_iter + 1));
  CS_HIP_CHECK(hipMemsetAsync(sums.p, 0, sizeof(unsigned long long) * ((size_t)n_prob * NS + 2), s));
  icp_launch_setup(est, c, st, s);
  if (est == ICP_GICP && c.mrmse) CS_HIP_CHECK(hipMemsetAsync(c.mrmse, 0, sizeof(double) * (size_t)n_prob, s));
  // the targets do not move: one image for every round
  ChfImage im;
  PoolBuf<int32_t> wflag;
  if (use_f16 && st.n_work)
    CS_REQUIRE(wflag.alloc(st.n_work) && im.pack(c.tgt, nt_rows, s), CS_ERR_HIP, "%s: scratch allocation failed", name);
  CS_LAUNCH_CHECK();
  st.img16 = im.img16.p;
  st.tn16 = im.tn16.p;
  st.t4f = im.t4f.p;
  st.wflag = wflag.p;
  for (int round = 0; round <= c.max_iter; ++round) {
    if (st.n_work) icp_launch_assoc(est, use_f16, c, st, s);
    icp_launch_step(est, c, st, round, round == c.max_iter ? 1 : 0, s);
  }
  CS_LAUNCH_CHECK();
  if (want_stats) {
    unsigned long long h[2] = {0, 0};
    CS_HIP_CHECK(download_async(h, dstats, sizeof(h), s));
    CS_HIP_CHECK(download_sync(s));
    g_icp_stats[0] += h[0];
    g_icp_stats[1] += h[1];
  }
  return CS_OK;
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

void cs_icp_stats(uint64_t out[2], int reset) { read_stats(g_icp_stats, out, reset); }

int cs_icp_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const int64_t* h_toff,
                 const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob, const float* d_T0, double max_dist,
                 int max_iter, double relative_fitness, double relative_rmse, double* d_T, float* d_T32,
                 double* d_fitness, double* d_rmse, int32_t* d_iters, int32_t* d_ncorr, int32_t* d_corr, void* stream) {
  IcpCall c{};
  c.src = d_src;
  c.soff = h_soff;
  c.tgt = d_tgt;
  c.toff = h_toff;
  c.src_seg = h_src_seg;
  c.tgt_seg = h_tgt_seg;
  c.n_prob = n_prob;
  c.T0 = d_T0;
  c.max_dist = max_dist;
  c.max_iter = max_iter;
  c.relative_fitness = relative_fitness;
  c.relative_rmse = relative_rmse;
  c.T = d_T;
  c.T32 = d_T32;
  c.fitness = d_fitness;
  c.rmse = d_rmse;
  c.iters = d_iters;
  c.ncorr = d_ncorr;
  c.corr = d_corr;
  c.stream = stream;
  return icp_run("cs_icp_batch", ICP_POINT, c);
}

int cs_icp_plane_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const float* d_tgt_normal,
                       const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob,
                       const float* d_T0, double max_dist, int max_iter, double relative_fitness, double relative_rmse,
                       double* d_T, float* d_T32, double* d_fitness, double* d_rmse, int32_t* d_iters, int32_t* d_ncorr,
                       int32_t* d_corr, void* stream) {
  IcpCall c{};
  c.src = d_src;
  c.soff = h_soff;
  c.tgt = d_tgt;
  c.tnrm = d_tgt_normal;
  c.toff = h_toff;
  c.src_seg = h_src_seg;
  c.tgt_seg = h_tgt_seg;
  c.n_prob = n_prob;
  c.T0 = d_T0;
  c.max_dist = max_dist;
  c.max_iter = max_iter;
  c.relative_fitness = relative_fitness;
  c.relative_rmse = relative_rmse;
  c.T = d_T;
  c.T32 = d_T32;
  c.fitness = d_fitness;
  c.rmse = d_rmse;
  c.iters = d_iters;
  c.ncorr = d_ncorr;
  c.corr = d_corr;
  c.stream = stream;
  return icp_run("cs_icp_plane_batch", ICP_PLANE, c);
}

int cs_icp_plane_robust_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const float* d_tgt_normal,
                              const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob,
                              const float* d_T0, double max_dist, int max_iter, double relative_fitness,
                              double relative_rmse, int kernel, double kernel_scale, double* d_T, float* d_T32,
                              double* d_fitness, double* d_rmse, double* d_wfitness, int32_t* d_iters, int32_t* d_ncorr,
                              int32_t* d_corr, void* stream) {
  const char* name = "cs_icp_plane_robust_batch";
  CS_REQUIRE(kernel >= CS_ICP_KERNEL_L2 && kernel <= CS_ICP_KERNEL_TUKEY, CS_ERR_INVALID, "%s: unknown kernel %d", name,
             kernel);
  IcpCall c{};
  c.src = d_src;
  c.soff = h_soff;
  c.tgt = d_tgt;
  c.tnrm = d_tgt_normal;
  c.toff = h_toff;
  c.src_seg = h_src_seg;
  c.tgt_seg = h_tgt_seg;
  c.n_prob = n_prob;
  c.T0 = d_T0;
  c.max_dist = max_dist;
  c.max_iter = max_iter;
  c.relative_fitness = relative_fitness;
  c.relative_rmse = relative_rmse;
  c.T = d_T;
  c.T32 = d_T32;
  c.fitness = d_fitness;
  c.rmse = d_rmse;
  c.wfitness = d_wfitness;
  c.iters = d_iters;
  c.ncorr = d_ncorr;
  c.corr = d_corr;
  c.stream = stream;
  if (kernel == CS_ICP_KERNEL_L2)   // every weight is 1: cs_icp_plane_batch's instantiation, the scale is ignored
    return icp_run(name, ICP_PLANE, c);
  CS_REQUIRE(std::isfinite(kernel_scale) && kernel_scale > 0.0, CS_ERR_INVALID,
             "%s: kernel_scale must be positive and finite", name);
  c.loss = IcpLoss{kernel, kernel_scale};
  return icp_run(name, ICP_ROBUST, c);
}

int cs_icp_scale_batch(const float* d_src, const int64_t* h_soff, const float* d_tgt, const float* d_tgt_normal,
                       const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob,
                       const float* d_T0, double max_dist, int max_iter, double relative_fitness, double relative_rmse,
                       double scale_min, double scale_max, double* d_T, float* d_T32, double* d_fitness, double* d_rmse,
                       double* d_scale, int32_t* d_iters, int32_t* d_ncorr, int32_t* d_corr, void* stream) {
  const char* name = "cs_icp_scale_batch";
  CS_REQUIRE(std::isfinite(scale_min) && std::isfinite(scale_max), CS_ERR_INVALID, "%s: a scale bound is not finite", name);
  CS_REQUIRE(scale_min > 0.0 && scale_min <= 1.0 && scale_max >= 1.0, CS_ERR_INVALID,
             "%s: the scale interval must satisfy 0 < scale_min <= 1 <= scale_max", name);
  IcpCall c{};
  c.src = d_src;
  c.soff = h_soff;
  c.tgt = d_tgt;
  c.tnrm = d_tgt_normal;   // NULL: point-to-point
  c.toff = h_toff;
  c.src_seg = h_src_seg;
  c.tgt_seg = h_tgt_seg;
  c.n_prob = n_prob;
  c.T0 = d_T0;
  c.max_dist = max_dist;
  c.max_iter = max_iter;
  c.relative_fitness = relative_fitness;
  c.relative_rmse = relative_rmse;
  c.scale_min = scale_min;
  c.scale_max = scale_max;
  c.T = d_T;
  c.T32 = d_T32;
  c.fitness = d_fitness;
  c.rmse = d_rmse;
  c.scale = d_scale;
  c.iters = d_iters;
  c.ncorr = d_ncorr;
  c.corr = d_corr;
  c.stream = stream;
  return icp_run(name, d_tgt_normal ? ICP_PLANE_S : ICP_POINT_S, c);
}

int cs_icp_gicp_batch(const float* d_src, const float* d_src_normal, const int64_t* h_soff, const float* d_tgt,
                      const float* d_tgt_normal, const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg,
                      int n_prob, const float* d_T0, double max_dist, int max_iter, double relative_fitness,
                      double relative_rmse, double epsilon, double* d_T, float* d_T32, double* d_fitness, double* d_rmse,
                      double* d_mrmse, int32_t* d_iters, int32_t* d_ncorr, int32_t* d_corr, void* stream) {
  const char* name = "cs_icp_gicp_batch";
  CS_REQUIRE(std::isfinite(epsilon) && epsilon >= 0x1.0p-10 && epsilon <= 1.0, CS_ERR_INVALID,
             "%s: epsilon must lie in [2^-10, 1]", name);
  IcpCall c{};
  c.src = d_src;
  c.snrm = d_src_normal;
  c.soff = h_soff;
  c.tgt = d_tgt;
  c.tnrm = d_tgt_normal;
  c.toff = h_toff;
  c.src_seg = h_src_seg;
  c.tgt_seg = h_tgt_seg;
  c.n_prob = n_prob;
  c.T0 = d_T0;
  c.max_dist = max_dist;
  c.max_iter = max_iter;
  c.relative_fitness = relative_fitness;
  c.relative_rmse = relative_rmse;
  c.epsilon = epsilon;
  c.T = d_T;
  c.T32 = d_T32;
  c.fitness = d_fitness;
  c.rmse = d_rmse;
  c.mrmse = d_mrmse;
  c.iters = d_iters;
  c.ncorr = d_ncorr;
  c.corr = d_corr;
  c.stream = stream;
  return icp_run(name, ICP_GICP, c);
}

}  // extern "C"
