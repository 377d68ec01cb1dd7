// The association of one ICP round: the posed ORIGINAL sources under the current T against the targets of
// their problem, the nearest target by (distance, row), and the sums of the kept pairs (icp_sums.h) at the end of either
// kernel.  k_icp_f16 ranks on the matrix cores and vouches for its result or flags its workgroup; k_icp_exact recomputes the
// flagged workgroups, and is the whole path under CS_ICP_F16=0.  icp_launch_assoc is the way in.
#include "icp.h"
#include "icp_sums.h"
#include "nn_common.h"

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

// The association on the f16 matrix cores: k_chamfer_f16's ranking (same image, same operand layout, same error budget;
// chamfer.hip and DESIGN 3 / 12) keeping (distance, row) of the evaluated rows and vouching STRICTLY: the result stands only
// when it lies below the smallest unevaluated tile minimum minus the error budget, so a row that was not evaluated can
// neither beat nor tie it.  A workgroup with a source that fails the test, or with coordinates outside the f16 range,
// adds nothing and raises its flag; k_icp_exact recomputes it.
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
  double px[CHF_NG], py[CHF_NG], pz[CHF_NG];
  f16x8 bop[CHF_NG];
  float b1[CHF_NG], b2[CHF_NG], b3[CHF_NG];
  int t1[CHF_NG], t2[CHF_NG];
  bool in_range = true;
#pragma unroll
  for (int g = 0; g < CHF_NG; ++g) {
    const int sloc = wave * 32 * CHF_NG + 32 * g + col;
    icp_pose(Tp, src + (wk.s0 + (sloc < wk.sn ? sloc : 0)) * 3, px[g], py[g], pz[g]);
    const float pf[3] = {(float)px[g] * CHF_SCALE, (float)py[g] * CHF_SCALE, (float)pz[g] * CHF_SCALE};
    _Float16 hi[3], lo[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      knf_split(-2.0f * pf[c], &hi[c], &lo[c]);
      in_range = in_range && fabsf(pf[c]) < 60.0f * CHF_SCALE;   // (NaN fails too)
    }
    // B rows k: 0..2 = -2 ph (x th), 3..5 = -2 ph (x tl), 6..8 = -2 pl (x th), 9..15 = 0; this lane holds k = 8 half .. + 7
    const _Float16 z0 = (_Float16)0.0f;
    if (half == 0)
      bop[g] = f16x8{hi[0], hi[1], hi[2], hi[0], hi[1], hi[2], lo[0], lo[1]};
    else
      bop[g] = f16x8{lo[2], z0, z0, z0, z0, z0, z0, z0};
    b1[g] = b2[g] = b3[g] = INFINITY;
    t1[g] = t2[g] = -1;
  }
  // register-staged double buffer of the 12-KiB image stages, as in k_chamfer_f16
  const uint4* gimg = reinterpret_cast<const uint4*>(img + pr.t0 * CHF_PITCH);
  constexpr int U4_PER_STAGE = CHF_ROWS * CHF_PITCH * 2 / 16;
  static_assert(U4_PER_STAGE == 3 * 256, "three 16-byte pieces per thread");
  uint4 st0, st1, st2;
  float stn;
  float tmax2 = 0.0f;
  auto load_stage = [&](int base) {
    const uint4* g = gimg + (int64_t)base * (CHF_PITCH * 2 / 16) + tid;
    st0 = g[0];
    st1 = g[256];
    st2 = g[512];
    const int r = base + tid;
    stn = r < tn ? tn32[pr.t0 + r] : INFINITY;   // rows past the segment (another problem's rows) never win
    if (r < tn) tmax2 = fmaxf(tmax2, stn);
  };
  auto store_stage = [&](int b) {
    uint4* d = reinterpret_cast<uint4*>(a_s[b]) + tid;
    d[0] = st0;
    d[256] = st1;
    d[512] = st2;
    tn_s[b][tid] = stn;
  };
  if (tn > 0) {
    load_stage(0);
    store_stage(0);
  }
  int buf = 0;
  for (int base = 0; base < tn; base += CHF_ROWS) {
    __syncthreads();
    const bool more = base + CHF_ROWS < tn;
    if (more) load_stage(base + CHF_ROWS);
#pragma unroll 1
    for (int t = 0; t < CHF_ROWS / 32; ++t) {
      if (base + 32 * t >= tn) break;   // whole tile past the range (block-uniform)
      const f16x8 a = *reinterpret_cast<const f16x8*>(a_s[buf] + (t * 32 + col) * CHF_PITCH + 8 * half);
      f32x16 c16;
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {
        const float4 v = *reinterpret_cast<const float4*>(&tn_s[buf][t * 32 + 8 * q4 + 4 * half]);
        c16[4 * q4 + 0] = v.x; c16[4 * q4 + 1] = v.y; c16[4 * q4 + 2] = v.z; c16[4 * q4 + 3] = v.w;
      }
      const int tile = base / 32 + t;
#pragma unroll
      for (int g = 0; g < CHF_NG; ++g) {
        const f32x16 d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop[g], c16, 0, 0, 0);
        float m = fminf(fminf(d[0], d[1]), d[2]);
        m = fminf(fminf(m, d[3]), d[4]);
        m = fminf(fminf(m, d[5]), d[6]);
        m = fminf(fminf(m, d[7]), d[8]);
        m = fminf(fminf(m, d[9]), d[10]);
        m = fminf(fminf(m, d[11]), d[12]);
        m = fminf(fminf(m, d[13]), d[14]);
        m = fminf(m, d[15]);
        const float o1 = b1[g], o2 = b2[g];
        const bool lt1 = m < o1, lt2 = m < o2;
        b1[g] = fminf(o1, m);
        b2[g] = __builtin_amdgcn_fmed3f(o1, o2, m);
        b3[g] = __builtin_amdgcn_fmed3f(o2, b3[g], m);
        t2[g] = lt1 ? t1[g] : (lt2 ? tile : t2[g]);
        t1[g] = lt1 ? tile : t1[g];
      }
    }
    if (more) store_stage(buf ^ 1);
    buf ^= 1;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) tmax2 = fmaxf(tmax2, __shfl_xor(tmax2, off));
  if (lane == 0) wmax[wave] = tmax2;
  __syncthreads();
  const double tmax = sqrt((double)fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))) / (double)CHF_SCALE;
  bool bad = !in_range || !(tmax < 60.0);
  const float4* trow = t4f + pr.t0;
  // canonical distances of this lane's 16 rows of a tile, ascending rows, strict <: the smallest by (distance, row)
  auto eval_tile = [&](int g, int tile, double& e, int& er) {
    e = INFINITY;
    er = 0x7fffffff;
    if (tile >= 0) {
      float4 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = tile * 32 + 4 * half + (i & 3) + 8 * (i >> 2);
        v[i] = trow[row < tn ? row : 0];
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = tile * 32 + 4 * half + (i & 3) + 8 * (i >> 2);
        const double dx = px[g] - (double)v[i].x, dy = py[g] - (double)v[i].y, dz = pz[g] - (double)v[i].z;
        const double d = fma(dz, dz, fma(dy, dy, dx * dx));
        if (row < tn && d < e) {
          e = d;
          er = row;
        }
      }
    }
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
    // error budget: the derivation in k_chamfer_f16 (the ranking value and its operands are the same)
    const double pn2 = fma(pz[g], pz[g], fma(py[g], py[g], px[g] * px[g]));
    const double S = (double)CHF_SCALE, PT = S * (sqrt(pn2) + tmax);
    const double eps = 0x1.0p-19 * PT * PT + 0x1.0p-10 * PT;
    double e;
    int er;
    eval_tile(g, t1[g], e, er);
    pair_min(e, er);
    float rest = fminf(b2[g], __shfl_xor(b2[g], 32));     // smallest unevaluated tile minimum of the source
    bool ok = rest == INFINITY || (e - pn2) * S * S < (double)rest - eps;
    if (__any(!ok)) {
      double e2 = INFINITY;
      int er2 = 0x7fffffff;
      if (!ok) eval_tile(g, t2[g], e2, er2);
      pair_min(e2, er2);
      if (!ok) {
        if (e2 < e || (e2 == e && er2 < er)) {
          e = e2;
          er = er2;
        }
        rest = fminf(b3[g], __shfl_xor(b3[g], 32));
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
  const double mpx = half ? px[1] : px[0], mpy = half ? py[1] : py[0], mpz = half ? pz[1] : pz[0];
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
