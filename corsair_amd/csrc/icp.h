// What the ICP units share: icp_sums.h (the specification of the sums), icp_assoc.hip (the two association
// kernels), icp_step.hip (set-up and the per-round step) and icp.hip (the host driver and the C entries).  The estimation is
// ONE axis, EST (0 = point, 1 = plane, 2 = plane with a per-pair weight, 3 = point + scale, 4 = plane + scale, 5 =
// plane-to-plane): a template argument of the sums at the end of the association kernels and of the update, a run-time int in
// the driver.  Its traits are constexpr functions of an int, so icp_nsum(EST) inside a kernel and icp_nsum(est) in the driver
// are the same function.  Every kernel is defined once, in one unit, and reached from the driver through an ordinary host
// function that picks the instantiation and launches on the stream it is given.
#pragma once
#include "common.h"

namespace cs {

constexpr int ICP_ST = 256;               // sources per workgroup (both association kernels): 4 waves x 32 x CHF_NG
constexpr int ICP_TT = 512;               // target rows per LDS stage of the exact kernel
constexpr int ICP_NSUM = 17;              // count, sum p' (3), sum q' (3), sum p' q'^T (9), sum d^2
constexpr int ICP_NSUM_PLANE = 29;        // count, sum J_i J_j (i <= j, 21), sum J_i r (6), sum d^2
constexpr int ICP_NSUM_ROBUST = 30;       // the 29 plane sums (27 of them weighted) + sum w
constexpr int ICP_NSUM_POINT_S = 18;      // the 17 point sums + sum p'.p'
constexpr int ICP_NSUM_PLANE_S = 37;      // count, sum J_i J_j (i <= j, 28), sum J_i r (7), sum d^2
constexpr int ICP_NSUM_GICP = 30;         // count, sum (J^T W J)_ij (i <= j, 21), sum (J^T W e)_i (6), sum d^2, sum e.We
constexpr int ICP_POINT = 0, ICP_PLANE = 1, ICP_ROBUST = 2, ICP_POINT_S = 3, ICP_PLANE_S = 4, ICP_GICP = 5;
// the estimations with a target normal array, the plane frame and the 6x6 / 7x7 normal equations: GICP's 30 sums have the
// plane layout (count, 21 matrix entries, 6 right-hand sides, d^2) with one more sum behind it
__host__ __device__ constexpr bool icp_is_plane(int est) {
  return est == ICP_PLANE || est == ICP_ROBUST || est == ICP_PLANE_S || est == ICP_GICP;
}
__host__ __device__ constexpr bool icp_has_scale(int est) { return est == ICP_POINT_S || est == ICP_PLANE_S; }
__host__ __device__ constexpr int icp_nsum(int est) {
  return est == ICP_ROBUST    ? ICP_NSUM_ROBUST
         : est == ICP_GICP    ? ICP_NSUM_GICP
         : est == ICP_PLANE   ? ICP_NSUM_PLANE
         : est == ICP_POINT_S ? ICP_NSUM_POINT_S
         : est == ICP_PLANE_S ? ICP_NSUM_PLANE_S
                              : ICP_NSUM;
}
// columns of the plane Jacobian: (a, n) and, with a scale, p'.n
__host__ __device__ constexpr int icp_nj(int est) { return est == ICP_PLANE_S ? 7 : 6; }
// sum d^2 is the 17th of both point layouts and the one after the J_i r sums of every plane layout (the 29th / 37th)
__host__ __device__ constexpr int icp_d2_at(int est) {
  return icp_is_plane(est) ? icp_nj(est) * (icp_nj(est) + 1) / 2 + icp_nj(est) + 1 : ICP_NSUM - 1;
}
// a rotational column of the plane Jacobian (bounded by 2 M) as opposed to a translational one (bounded by 1)
__host__ __device__ constexpr bool icp_rot_col(int i) { return i < 3 || i == 6; }

// the exponent range of M and the bits of a sum: icp_sums.h has the derivation, k_icp_frame (icp_step.hip) applies it
constexpr int ICP_EM_MIN = -100;
constexpr int ICP_EM_MAX = 400;
constexpr int ICP_SUM_BITS = 61;

struct IcpProb {
  int64_t s0, t0;   // first source / target row (global)
  int64_t c0;       // first entry of the problem in d_corr
  int32_t sn, tn;
};
struct IcpWork {
  int64_t s0;       // first source row of this workgroup (global)
  int64_t c0;       // its first entry in d_corr
  int32_t sn;       // source rows (<= ICP_ST)
  int32_t prob;
};
struct IcpFrame {
  double o[3];      // origin: midpoint of the target segment's bounding box
  double sc1, sc2;  // 2^s1, 2^s2
  double inv1, inv2;
  double clamp;     // 2^(61 - eN)
  double sc_pp, inv_pp;   // 2^(s2 - 2) and its inverse: the sum of p'.p' (EST = 3)
};
struct IcpPlaneFrame {   // 2^s and 2^-s of the five product classes of the plane sums
  double sc_rr, inv_rr, sc_rt, inv_rt, sc_tt, inv_tt, sc_rd, inv_rd, sc_td, inv_td;
};
struct IcpLoss {     // the robust kernel of EST = 2 (CS_ICP_KERNEL_*), unused otherwise
  int kind;
  double k;          // kernel_scale
};
struct IcpCriteria {
  double thr2;      // max_dist * max_dist
  double rel_fitness, rel_rmse;
  double scale_min, scale_max;   // the interval of the accumulated scale (EST = 3, 4)
};

// One call of any entry: the arguments the five entries share under the names of include/corsair_hip.h (without the d_ / h_
// prefixes), then what only some of them have, with the value that means "not this entry".
struct IcpCall {
  const float* src;
  const int64_t* soff;
  const float* tgt;
  const int64_t* toff;
  const int32_t *src_seg, *tgt_seg;
  int n_prob;
  const float* T0;
  double max_dist;
  int max_iter;
  double relative_fitness, relative_rmse;
  double* T;
  float* T32;
  double *fitness, *rmse;
  int32_t *iters, *ncorr, *corr;
  void* stream;
  const float* tnrm = nullptr;                // the target normals of the plane estimations (EST = 1, 2, 4, 5)
  const float* snrm = nullptr;                // the source normals of cs_icp_gicp_batch (EST = 5)
  IcpLoss loss = {CS_ICP_KERNEL_L2, 0.0};     // the kernel of EST = 2
  double* wfitness = nullptr;                 // the optional weighted inlier share of cs_icp_plane_robust_batch
  double scale_min = 1.0, scale_max = 1.0;    // the interval and the output of cs_icp_scale_batch (EST = 3, 4)
  double* scale = nullptr;
  double epsilon = 1.0;                       // the covariance floor and the optional Mahalanobis rmse of EST = 5
  double* mrmse = nullptr;
};

// What the driver derives and allocates for a call, as the launch functions take it.
struct IcpState {
  const IcpProb* probs;
  const IcpWork* work;
  unsigned n_work;
  IcpFrame* frame;
  IcpPlaneFrame* pframe;        // NULL unless icp_is_plane(est)
  unsigned long long* sums;     // n_prob * icp_nsum(est)
  unsigned long long* stats;    // the two counters of CS_ICP_STATS behind the sums, NULL when they are not wanted
  int32_t* done;
  // the f16 image of the targets (ChfImage, chf_rank.h) and the workgroup flags: NULL under CS_ICP_F16=0
  const _Float16* img16;
  const float* tn16;
  const float4* t4f;
  int32_t* wflag;
  IcpCriteria crit;
  double ome;                   // GICP: 1 - epsilon
  int eW;                       // GICP: the exponent the plane scales give up to the weight matrix (0 otherwise)
};

// icp_step.hip.  Set-up: k_icp_init (outputs and T from T0), then k_icp_frame (the fixed-point frames of every problem).
void icp_launch_setup(int est, const IcpCall& c, const IcpState& w, hipStream_t s);
// k_icp_step<est> of one round; last: the round after the max_iter-th update
void icp_launch_step(int est, const IcpCall& c, const IcpState& w, int round, int last, hipStream_t s);
// icp_assoc.hip.  A round's association: k_icp_f16<est>, then k_icp_exact<est> over the workgroups it flagged, or
// k_icp_exact<est> alone
void icp_launch_assoc(int est, bool use_f16, const IcpCall& c, const IcpState& w, hipStream_t s);

}  // namespace cs
