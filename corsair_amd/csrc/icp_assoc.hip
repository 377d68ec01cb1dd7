// The association of one ICP round: the posed ORIGINAL sources under the current T against the targets of
// their problem, the nearest target by (distance, row), and the sums of the kept pairs (icp_sums.h) at the end of either
// kernel.  k_icp_f16 ranks on the matrix cores (chf_rank.h: the scan it shares with k_chamfer_f16) and vouches for its result
// or flags its workgroup; k_icp_exact recomputes the flagged workgroups, and is the whole path under CS_ICP_F16=0.
// icp_launch_assoc is the way in.
#include "chf_rank.h"
#include "icp.h"
#include "icp_sums.h"

namespace cs {
namespace {

static_assert(ICP_ST == 4 * 32 * CHF_NG, "a workgroup's sources are the columns of its four waves' MFMA groups");

// Exhaustive association, one source per thread: the canonical chain over every target row in ascending order with a
// strict comparison, i.e. the minimum by (distance, row).  The whole path under CS_ICP_F16=0, and the recomputation of
// the workgroups k_icp_f16 flags.
template <int EST>
__global__ __launch_bounds__(256) void k_icp_exact(const IcpWork* __restrict__ work, const IcpProb* __restrict__ probs,
                                                   const float* __restrict__ src, const float* __restrict__ tgt,
                                                   const float* __restrict__ tnrm, const double* __restrict__ T,
                                                   const IcpFrame* __restrict__ frame,
                                                   const IcpPlaneFrame* __restrict__ pframe,
                                                   const int32_t* __restrict__ done, double thr2,
                                                   IcpLoss loss, unsigned long long* __restrict__ sums,
                                                   int32_t* __restrict__ corr,
                                                   const int32_t* __restrict__ only_flagged,
                                                   const float* __restrict__ snrm, double ome) {
  __shared__ float t_lds[ICP_TT * 3];
  __shared__ unsigned long long part[4][icp_nsum(EST)];
  if (only_flagged && !only_flagged[blockIdx.x]) return;
  const IcpWork wk = work[blockIdx.x];
  if (done[wk.prob]) return;
  const IcpProb pr = probs[wk.prob];
  const int tid = threadIdx.x;
  const bool active = tid < wk.sn;
  double px = 0, py = 0, pz = 0;
  if (active) icp_pose(T + (int64_t)wk.prob * 16, src + (wk.s0 + tid) * 3, px, py, pz);
  double best = INFINITY;
  int bidx = -1;
  for (int tbase = 0; tbase < pr.tn; tbase += ICP_TT) {
    const int tcount = min(ICP_TT, pr.tn - tbase);
    __syncthreads();
    for (int i = tid; i < tcount * 3; i += 256) t_lds[i] = tgt[(pr.t0 + tbase) * 3 + i];
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < tcount; ++j) {
      const double dx = px - (double)t_lds[3 * j + 0];
      const double dy = py - (double)t_lds[3 * j + 1];
      const double dz = pz - (double)t_lds[3 * j + 2];
      const double d = fma(dz, dz, fma(dy, dy, dx * dx));
      if (d < best) {
        best = d;
        bidx = tbase + j;
      }
    }
  }
  const bool kept = active && bidx >= 0 && best < thr2;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (kept) {
    const float* tp = tgt + (pr.t0 + bidx) * 3;
    qx = tp[0];
    qy = tp[1];
    qz = tp[2];
  }
  if (corr && active) corr[wk.c0 + tid] = kept ? bidx : -1;
  icp_block_sums<EST>(kept, px, py, pz, qx, qy, qz, best, frame[wk.prob], icp_is_plane(EST) ? pframe + wk.prob : nullptr,
                      icp_is_plane(EST) && kept ? tnrm + (pr.t0 + bidx) * 3 : nullptr, loss,
                      sums + (int64_t)wk.prob * icp_nsum(EST), part,
                      EST == ICP_GICP && kept ? snrm + (wk.s0 + tid) * 3 : nullptr, T + (int64_t)wk.prob * 16, ome);
}

// The association on the f16 matrix cores: the ranking scan of chf_rank.h, which k_chamfer_f16 runs as well (same image,
// same operands, same error budget), keeping (distance, row) of the evaluated rows and vouching STRICTLY:
// the result stands only when it lies below the smallest unevaluated tile minimum minus the error budget, so a row that
// was not evaluated can neither beat nor tie it.  A workgroup with a source that fails the test, or with coordinates
// outside the f16 range, adds nothing and raises its flag; k_icp_exact recomputes it.
template <int EST>
__global__ __launch_bounds__(256) void k_icp_f16(const IcpWork* __restrict__ work, const IcpProb* __restrict__ probs,
                                                 const float* __restrict__ src, const float4* __restrict__ t4f,
                                                 const _Float16* __restrict__ img, const float* __restrict__ tn32,
                                                 const float* __restrict__ tnrm, const double* __restrict__ T,
                                                 const IcpFrame* __restrict__ frame,
                                                 const IcpPlaneFrame* __restrict__ pframe,
                                                 const int32_t* __restrict__ done, double thr2,
                                                 IcpLoss loss, unsigned long long* __restrict__ sums,
                                                 int32_t* __restrict__ corr, int32_t* __restrict__ flag,
                                                 unsigned long long* __restrict__ stats,
                                                 const float* __restrict__ snrm, double ome) {
  __shared__ __attribute__((aligned(16))) _Float16 a_s[2][CHF_ROWS * CHF_PITCH];
  __shared__ __attribute__((aligned(16))) float tn_s[2][CHF_ROWS];
  __shared__ unsigned long long part[4][icp_nsum(EST)];
  __shared__ float wmax[4];
  __shared__ int wg_bad;
  const IcpWork wk = work[blockIdx.x];
  const int tid = threadIdx.x;
  if (done[wk.prob]) {
    if (tid == 0) flag[blockIdx.x] = 0;
    return;
  }
  const IcpProb pr = probs[wk.prob];
  const int tn = pr.tn;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int half = lane >> 5;
  const int col = lane & 31;
  const double* Tp = T + (int64_t)wk.prob * 16;
  if (tid == 0) wg_bad = 0;
  ChfRank rk;
#pragma unroll
  for (int g = 0; g < CHF_NG; ++g) {
    const int sloc = wave * 32 * CHF_NG + 32 * g + col;
    icp_pose(Tp, src + (wk.s0 + (sloc < wk.sn ? sloc : 0)) * 3, rk.px[g], rk.py[g], rk.pz[g]);
    chf_operand(rk, g, half);
  }
  // (block-uniform: the early return on done[prob] above is taken by the whole workgroup)
  const double tmax = chf_scan(rk, img, tn32, pr.t0, tn, a_s, tn_s, wmax, tid);
  bool bad = !rk.in_range || !(tmax < 60.0);
  const float4* trow = t4f + pr.t0;
  // this lane's 16 rows of a tile: the smallest by (distance, row)
  auto eval_tile = [&](int g, int tile, double& e, int& er) {
    chf_eval_tile(trow, tn, tile, half, rk.px[g], rk.py[g], rk.pz[g], e, er);
  };
  // (distance, row) minimum of the two lanes of a source
  auto pair_min = [&](double& e, int& er) {
    const double oe = __shfl_xor(e, 32);
    const int orow = __shfl_xor(er, 32);
    if (oe < e || (oe == e && orow < er)) {
      e = oe;
      er = orow;
    }
  };
  double my_e = INFINITY;
  int my_row = 0x7fffffff;
#pragma unroll
  for (int g = 0; g < CHF_NG; ++g) {
    const double pn2 = fma(rk.pz[g], rk.pz[g], fma(rk.py[g], rk.py[g], rk.px[g] * rk.px[g]));
    const double S = (double)CHF_SCALE, eps = chf_eps(pn2, tmax);
    // vouching with a strict < (k_chamfer_f16: <=): the row is returned, and an unevaluated row that ties could be the smaller
    double e;
    int er;
    eval_tile(g, rk.t1[g], e, er);
    pair_min(e, er);
    float rest = fminf(rk.b2[g], __shfl_xor(rk.b2[g], 32));     // smallest unevaluated tile minimum of the source
    bool ok = rest == INFINITY || (e - pn2) * S * S < (double)rest - eps;
    if (__any(!ok)) {
      double e2 = INFINITY;
      int er2 = 0x7fffffff;
      if (!ok) eval_tile(g, rk.t2[g], e2, er2);
      pair_min(e2, er2);
      if (!ok) {
        if (e2 < e || (e2 == e && er2 < er)) {
          e = e2;
          er = er2;
        }
        rest = fminf(rk.b3[g], __shfl_xor(rk.b3[g], 32));
        ok = rest == INFINITY || (e - pn2) * S * S < (double)rest - eps;
      }
    }
    const int sloc = wave * 32 * CHF_NG + 32 * g + col;
    if (sloc < wk.sn && !ok) bad = true;
    if (g == half) {       // both lanes of a source hold its result: lane `half` carries the source of group `half`
      my_e = e;
      my_row = er;
    }
  }
  static_assert(CHF_NG == 2, "one source per thread in the sums: group g is carried by the lanes of half g");
  if (__any(bad) && lane == 0) atomicOr(&wg_bad, 1);
  __syncthreads();
  const int wbad = wg_bad;
  if (tid == 0) {
    flag[blockIdx.x] = wbad;
    if (stats) {
      atomicAdd(&stats[0], 1ULL);
      if (wbad) atomicAdd(&stats[1], 1ULL);
    }
  }
  if (wbad) return;   // block-uniform
  const double mpx = half ? rk.px[1] : rk.px[0], mpy = half ? rk.py[1] : rk.py[0], mpz = half ? rk.pz[1] : rk.pz[0];
  const bool active = tid < wk.sn;   // sloc of (wave, g = half, col) = tid
  const bool kept = active && my_row != 0x7fffffff && my_e < thr2;
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (kept) q = trow[my_row];
  if (corr && active) corr[wk.c0 + tid] = kept ? my_row : -1;
  icp_block_sums<EST>(kept, mpx, mpy, mpz, q.x, q.y, q.z, my_e, frame[wk.prob],
                      icp_is_plane(EST) ? pframe + wk.prob : nullptr,
                      icp_is_plane(EST) && kept ? tnrm + (pr.t0 + my_row) * 3 : nullptr, loss,
                      sums + (int64_t)wk.prob * icp_nsum(EST), part,
                      EST == ICP_GICP && kept ? snrm + (wk.s0 + tid) * 3 : nullptr, Tp, ome);
}

// k_icp_exact runs over the workgroups k_icp_f16 has just flagged, or over every workgroup when it is alone
template <int EST>
void launch_assoc(bool use_f16, const IcpCall& c, const IcpState& w, hipStream_t s) {
  if (use_f16)
    hipLaunchKernelGGL(k_icp_f16<EST>, dim3(w.n_work), dim3(256), 0, s, w.work, w.probs, c.src, w.t4f, w.img16, w.tn16,
                       c.tnrm, (const double*)c.T, w.frame, w.pframe, w.done, w.crit.thr2, c.loss, w.sums, c.corr, w.wflag,
                       w.stats, c.snrm, w.ome);
  hipLaunchKernelGGL(k_icp_exact<EST>, dim3(w.n_work), dim3(256), 0, s, w.work, w.probs, c.src, c.tgt, c.tnrm,
                     (const double*)c.T, w.frame, w.pframe, w.done, w.crit.thr2, c.loss, w.sums, c.corr,
                     use_f16 ? (const int32_t*)w.wflag : (const int32_t*)nullptr, c.snrm, w.ome);
}

}  // namespace

void icp_launch_assoc(int est, bool use_f16, const IcpCall& c, const IcpState& w, hipStream_t s) {
  switch (est) {
    case ICP_POINT: return launch_assoc<ICP_POINT>(use_f16, c, w, s);
    case ICP_PLANE: return launch_assoc<ICP_PLANE>(use_f16, c, w, s);
    case ICP_ROBUST: return launch_assoc<ICP_ROBUST>(use_f16, c, w, s);
    case ICP_POINT_S: return launch_assoc<ICP_POINT_S>(use_f16, c, w, s);
    case ICP_PLANE_S: return launch_assoc<ICP_PLANE_S>(use_f16, c, w, s);
    case ICP_GICP: return launch_assoc<ICP_GICP>(use_f16, c, w, s);
  }
}

}  // namespace cs
