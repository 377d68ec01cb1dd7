// One-directional Chamfer and Hausdorff distances of posed clouds, exact in f64 so that the values equal those of the
// reference's SciPy routine:
//   cs_chamfer_1dir / cs_hausdorff_1dir <- apply_transform + KDTree 1-NN   (utils/preprocess.py:39-48,67-70)
// The canonical distance of a source p = R s + t to a target is the f64 fma chain over x, y, z; the result of a source is
// the minimum over the targets.  Every distance that enters a sum or maximum is that of the canonical chain; the fast
// paths only decide WHICH targets get the canonical evaluation:
//   * default: k_chamfer_f16 ranks by |t|^2 - 2 p.t on the f16 matrix cores (chf_rank.h: the scan it shares with the ICP's
//     k_icp_f16), evaluates the rows of the two best tiles with the canonical chain and vouches for the result against
//     the scan's error budget; workgroups it cannot vouch for are recomputed by k_chamfer_mfma (flag array, no host
//     decision).  CS_CHAMFER_STATS=1 counts those workgroups (cs_chamfer_f16_stats; synchronises).
//   * CS_CHAMFER_F16=0: k_chamfer_mfma for every tile -- arg-min on the f64 matrix pipe, canonical chain on the four
//     candidates of a source.
//   * CS_CHAMFER_MFMA=0: k_chamfer, exhaustive on the VALU -- what the tests hold the other two against.
// k_chamfer_finish turns the tiles' partial results into the mean (Chamfer) or maximum (Hausdorff) of each problem.
// Non-finite rows (include/corsair_hip.h): a target at NaN or +inf distance is never the nearest -- every search keeps its
// best with a strict `<` from +inf, the tile minima are fminf / v_min3 (a NaN operand loses), fmin drops a NaN canonical
// distance.  A source without a target at finite distance keeps +inf, and the problem's sum or maximum is +inf.  The f16
// kernel cannot vouch for a source or pose that is not finite (in_range), nor for a segment with an infinite or huge row
// (tmax; a NaN row does not enter it): those workgroups go to k_chamfer_mfma.
// cs_chamfer_2dir (both directions under one pose, the score of the candidate verification) has one path:
// k_chamfer2, exhaustive on the VALU like k_chamfer, each direction searched with its own rows in registers.
#include <algorithm>

#include "chf_rank.h"

namespace cs {

// the posed source of every kernel here
__device__ __forceinline__ void chamfer_pose(const float* __restrict__ Tp, const float* __restrict__ s, double* px,
                                             double* py, double* pz) {
  const double x = s[0], y = s[1], z = s[2];
  // row-major 4x4: p = R x + t, evaluated as fma(r0,x, fma(r1,y, fma(r2,z, t)))
  *px = fma((double)Tp[0], x, fma((double)Tp[1], y, fma((double)Tp[2], z, (double)Tp[3])));
  *py = fma((double)Tp[4], x, fma((double)Tp[5], y, fma((double)Tp[6], z, (double)Tp[7])));
  *pz = fma((double)Tp[8], x, fma((double)Tp[9], y, fma((double)Tp[10], z, (double)Tp[11])));
}

// The tail of every search kernel: red[0, N) holds a value per source (0 for a thread without one); afterwards red[0] is
// their sum, or their maximum.  Contains barriers: the whole workgroup calls it.
template <int N>
__device__ __forceinline__ void chamfer_block_reduce(double (&red)[N], int tid, int reduce_max) {
  __syncthreads();
  for (int off = N / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] = reduce_max ? fmax(red[tid], red[tid + off]) : red[tid] + red[tid + off];
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// one-directional Chamfer
// ------------------------------------------------------------------------------------------
struct ChamferWork {
  int64_t s0;   // first source row of this tile (global)
  int64_t t0;   // first target row (global)
  int32_t sn;   // source rows in this tile (<= 256)
  int32_t tn;   // target rows
  int32_t prob;
  int32_t slot; // index into the partial-sum array
};

constexpr int CH_TT = 512;

__global__ __launch_bounds__(256) void k_chamfer(const ChamferWork* __restrict__ work,
                                                 const float* __restrict__ src,
                                                 const float* __restrict__ tgt,
                                                 const float* __restrict__ T, int reduce_max,
                                                 double* __restrict__ partial) {
  __shared__ float t_lds[CH_TT * 3];
  __shared__ double red[256];
  const ChamferWork wk = work[blockIdx.x];
  const int tid = threadIdx.x;
  const bool active = tid < wk.sn;
  const float* Tp = T + (int64_t)wk.prob * 16;
  double px = 0, py = 0, pz = 0;
  if (active) chamfer_pose(Tp, src + (wk.s0 + tid) * 3, &px, &py, &pz);
  double best = INFINITY;
  for (int tbase = 0; tbase < wk.tn; tbase += CH_TT) {
    const int tcount = min(CH_TT, wk.tn - tbase);
    __syncthreads();
    for (int i = tid; i < tcount * 3; i += 256) t_lds[i] = tgt[(wk.t0 + tbase) * 3 + i];
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < tcount; ++j) {
      double dx = px - (double)t_lds[3 * j + 0];
      double dy = py - (double)t_lds[3 * j + 1];
      double dz = pz - (double)t_lds[3 * j + 2];
      double d = fma(dz, dz, fma(dy, dy, dx * dx));
      best = d < best ? d : best;
    }
  }
  red[tid] = active ? sqrt(best) : 0.0;
  chamfer_block_reduce(red, tid, reduce_max);
  if (tid == 0) partial[wk.slot] = red[0];
}

// The same search on the f64 matrix pipe: A = [tx, ty, tz, |t|^2] (targets, LDS), B = [-2px, -2py, -2pz, 1]
// (transformed sources, registers): one v_mfma_f64_16x16x4_f64 gives |t|^2 - 2 p.t for 16 x 16 pairs,
// the ranking value of each source.  Every lane keeps the arg-min of its quarter of the targets, the
// four candidates of a source are re-evaluated with the canonical chain and the smallest is the
// result -- equal to the exhaustive chain unless two targets are within the expansion's rounding
// (~5e-16 absolute in d^2) of the minimum, where the two values differ by less than that.
constexpr int CHM_NG = 4;               // 16-source groups per wave: every staged target row serves 256 sources
constexpr int CHM_ST = 64 * CHM_NG;     // sources per workgroup
constexpr int CHM_TT = 512;             // targets per LDS stage
// A-operand rows of every target, once per call: (x, y, z, |t|^2) in f64
__global__ void k_chamfer_pack(const float* __restrict__ tgt, int64_t n, double* __restrict__ t4g) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = tgt[3 * i], y = tgt[3 * i + 1], z = tgt[3 * i + 2];
  double* o = t4g + 4 * i;
  o[0] = x;
  o[1] = y;
  o[2] = z;
  o[3] = fma(z, z, fma(y, y, x * x));
}

__global__ __launch_bounds__(256) void k_chamfer_mfma(const ChamferWork* __restrict__ work,
                                                      const float* __restrict__ src,
                                                      const float* __restrict__ tgt,
                                                      const double* __restrict__ t4g,
                                                      const float* __restrict__ T, int reduce_max,
                                                      double* __restrict__ partial,
                                                      // != nullptr: only the tiles the f16 kernel could not vouch for
                                                      const int32_t* __restrict__ only_flagged) {
  __shared__ __attribute__((aligned(16))) double t4[CHM_TT * 4];
  __shared__ double red[CHM_ST];
  if (only_flagged && !only_flagged[blockIdx.x]) return;
  const ChamferWork wk = work[blockIdx.x];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int col = lane & 15;  // source within a group (B side); target row within a 16-row tile (A side)
  const int kq = lane >> 4;   // k slot of the operands; row group of the results
  const float* Tp = T + (int64_t)wk.prob * 16;
  double px[CHM_NG], py[CHM_NG], pz[CHM_NG], bq[CHM_NG], best[CHM_NG];
  int bidx[CHM_NG];
#pragma unroll
  for (int g = 0; g < CHM_NG; ++g) {
    const int sloc = (wave * CHM_NG + g) * 16 + col;
    chamfer_pose(Tp, src + (wk.s0 + (sloc < wk.sn ? sloc : 0)) * 3, &px[g], &py[g], &pz[g]);
    bq[g] = kq == 0 ? -2.0 * px[g] : (kq == 1 ? -2.0 * py[g] : (kq == 2 ? -2.0 * pz[g] : 1.0));
    best[g] = INFINITY;
    bidx[g] = -1;
  }
  for (int tbase = 0; tbase < wk.tn; tbase += CHM_TT) {
    const int tcount = min(CHM_TT, wk.tn - tbase);
    __syncthreads();
    for (int j = tid; j < CHM_TT; j += 256) {
      double2 xy = make_double2(0.0, 0.0), zn = make_double2(0.0, INFINITY);  // rows past the segment never win
      if (j < tcount) {
        const double2* tp = reinterpret_cast<const double2*>(t4g + (wk.t0 + tbase + j) * 4);
        xy = tp[0];
        zn = tp[1];
      }
      *reinterpret_cast<double2*>(&t4[4 * j]) = xy;
      *reinterpret_cast<double2*>(&t4[4 * j + 2]) = zn;
    }
    __syncthreads();
    for (int t = 0; t < (tcount + 15) / 16; ++t) {
      const double a = t4[(16 * t + col) * 4 + kq];
#pragma unroll
      for (int g = 0; g < CHM_NG; ++g) {
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bq[g], acc, 0, 0, 0);
        // acc[r] = |t|^2 - 2 p.t of target row 16 t + kq + 4 r and source col of group g
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (acc[r] < best[g]) {
            best[g] = acc[r];
            bidx[g] = tbase + 16 * t + kq + 4 * r;
          }
        }
      }
    }
  }
  // canonical distance of this lane's candidate, then the smallest of the source's four lanes
#pragma unroll
  for (int g = 0; g < CHM_NG; ++g) {
    double d = INFINITY;
    if (bidx[g] >= 0) {
      const float* tp = tgt + (wk.t0 + bidx[g]) * 3;
      const double dx = px[g] - (double)tp[0], dy = py[g] - (double)tp[1], dz = pz[g] - (double)tp[2];
      d = fma(dz, dz, fma(dy, dy, dx * dx));
    }
    d = fmin(d, __shfl_xor(d, 16));
    d = fmin(d, __shfl_xor(d, 32));
    const int sloc = (wave * CHM_NG + g) * 16 + col;
    if (kq == 0) red[sloc] = sloc < wk.sn ? sqrt(d) : 0.0;
  }
  chamfer_block_reduce(red, tid, reduce_max);
  if (tid == 0) partial[wk.slot] = red[0];
}

// ------------------------------------------------------------------------------------------
// The same search on the f16 matrix cores (round 5).  The f64 matrix pipe of gfx950 is the vector unit's double-precision
// ALU (78.6 TF either way): k_chamfer_mfma sits at 0.23 of it with five VALU operations per result on top.  The ranking
// value |t|^2 - 2 p.t needs nine products when the coordinates are cut into f16 hi + lo (ph.th + ph.tl + pl.th): ONE
// v_mfma_f32_32x32x16_f16 per 32 targets x 32 sources with |t|^2 in the accumulator input, 16x the rate per pair.  It only
// RANKS (chf_rank.h: image, operands, scan and error budget, shared with the ICP's association kernel): at the end the
// rows of a lane's two best tiles are evaluated with the canonical f64 chain, and the result is vouched for when it lies
// below the smallest unevaluated tile minimum minus the error budget -- then no row outside the evaluated tiles can be
// nearer.  A workgroup with a source that fails the test is recomputed by k_chamfer_mfma (flag array, no host decision).
// Coordinates outside the f16 range (|coordinate| >= 60) take the f64 kernel as well.  Results: the same canonical
// distances as the other two kernels (tests/test_gpu_post.py::test_chamfer_matches_oracle, all three paths).
static_assert(4 * 32 * CHF_NG == CHM_ST, "the f16 kernel and its f64 fallback share the work items");

// the target image of chf_rank.h; rows [n, n_pad) are zero with tn32 = +inf (they never win)
__global__ void k_chamfer_pack16(const float* __restrict__ tgt, int64_t n, int64_t n_pad, _Float16* __restrict__ img,
                                 float* __restrict__ tn32, float4* __restrict__ t4f) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n_pad) return;
  union {
    _Float16 h[CHF_PITCH];
    uint4 v[3];
  } row;
#pragma unroll
  for (int c = 0; c < CHF_PITCH; ++c) row.h[c] = (_Float16)0.0f;
  float t2 = INFINITY;
  if (i < n) {
    // (x, y, z, 0) in one 16-byte row: the final canonical evaluation reads a candidate row with ONE request instead of three
    t4f[i] = make_float4(tgt[3 * i], tgt[3 * i + 1], tgt[3 * i + 2], 0.0f);
    double n2 = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = tgt[3 * i + c] * CHF_SCALE;     // exact (power of two) unless it overflows, which the kernel flags
      _Float16 hi, lo;
      knf_split(v, &hi, &lo);
      row.h[c] = hi;
      row.h[3 + c] = lo;
      row.h[6 + c] = hi;
      n2 = fma((double)v, (double)v, n2);
    }
    t2 = (float)n2;
  }
  uint4* dst = reinterpret_cast<uint4*>(img + i * CHF_PITCH);
#pragma unroll
  for (int c = 0; c < 3; ++c) dst[c] = row.v[c];
  tn32[i] = t2;
}

__global__ __launch_bounds__(256) void k_chamfer_f16(const ChamferWork* __restrict__ work, const float* __restrict__ src,
                                                     const float4* __restrict__ t4f, const _Float16* __restrict__ img,
                                                     const float* __restrict__ tn32, const float* __restrict__ T,
                                                     int reduce_max, double* __restrict__ partial,
                                                     int32_t* __restrict__ flag) {
  __shared__ __attribute__((aligned(16))) _Float16 a_s[2][CHF_ROWS * CHF_PITCH];
  __shared__ __attribute__((aligned(16))) float tn_s[2][CHF_ROWS];
  __shared__ double red[CHM_ST];
  __shared__ float wmax[4];
  __shared__ int wg_bad;
  const ChamferWork wk = work[blockIdx.x];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int half = lane >> 5;
  const int col = lane & 31;
  const float* Tp = T + (int64_t)wk.prob * 16;
  if (tid == 0) wg_bad = 0;
  ChfRank rk;
#pragma unroll
  for (int g = 0; g < CHF_NG; ++g) {
    const int sloc = wave * 32 * CHF_NG + 32 * g + col;
    chamfer_pose(Tp, src + (wk.s0 + (sloc < wk.sn ? sloc : 0)) * 3, &rk.px[g], &rk.py[g], &rk.pz[g]);
    chf_operand(rk, g, half);
  }
  const double tmax = chf_scan(rk, img, tn32, wk.t0, wk.tn, a_s, tn_s, wmax, tid);
  bool bad = !rk.in_range || !(tmax < 60.0);
  const float4* trow = t4f + wk.t0;
  auto eval_tile = [&](int g, int tile) {   // smallest canonical distance of this lane's 16 rows of a tile
    double e;
    int er;
    chf_eval_tile(trow, wk.tn, tile, half, rk.px[g], rk.py[g], rk.pz[g], e, er);
    return e;
  };
#pragma unroll
  for (int g = 0; g < CHF_NG; ++g) {
    const double pn2 = fma(rk.pz[g], rk.pz[g], fma(rk.py[g], rk.py[g], rk.px[g] * rk.px[g]));
    const double S = (double)CHF_SCALE, eps = chf_eps(pn2, tmax);
    // best tile of either lane of the source first; the second tiles only where that does not settle it.  Vouching with
    // <= (k_icp_f16: <): an unevaluated row that ties has the same distance, and only the distance is returned here.
    double e = eval_tile(g, rk.t1[g]);
    e = fmin(e, __shfl_xor(e, 32));
    float rest = fminf(rk.b2[g], __shfl_xor(rk.b2[g], 32));     // smallest unevaluated tile minimum of the source
    bool ok = rest == INFINITY || (e - pn2) * S * S <= (double)rest - eps;
    if (__any(!ok)) {
      double e2 = ok ? INFINITY : eval_tile(g, rk.t2[g]);
      e2 = fmin(e2, __shfl_xor(e2, 32));
      if (!ok) {
        e = fmin(e, e2);
        rest = fminf(rk.b3[g], __shfl_xor(rk.b3[g], 32));
        ok = rest == INFINITY || (e - pn2) * S * S <= (double)rest - eps;
      }
    }
    const int sloc = wave * 32 * CHF_NG + 32 * g + col;
    if (sloc < wk.sn && !ok) bad = true;
    if (half == 0) red[sloc] = sloc < wk.sn ? sqrt(e) : 0.0;
  }
  if (__any(bad) && lane == 0) atomicOr(&wg_bad, 1);
  chamfer_block_reduce(red, tid, reduce_max);
  if (tid == 0) {
    partial[wk.slot] = red[0];
    flag[blockIdx.x] = wg_bad;
  }
}

void chamfer_pack16(const float* d_tgt, int64_t n, int64_t n_pad, _Float16* img, float* tn32, float4* t4f, hipStream_t s) {
  hipLaunchKernelGGL(k_chamfer_pack16, dim3((unsigned)ceil_div(n_pad, 256)), dim3(256), 0, s, d_tgt, n, n_pad, img, tn32,
                     t4f);
}

__global__ void k_chamfer_finish(const double* __restrict__ partial,
                                 const int32_t* __restrict__ slot_begin,
                                 const int64_t* __restrict__ src_count, int n_prob, int reduce_max,
                                 double* __restrict__ out) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  double s = 0.0;
  for (int i = slot_begin[p]; i < slot_begin[p + 1]; ++i)
    s = reduce_max ? fmax(s, partial[i]) : s + partial[i];
  if (reduce_max)
    out[p] = src_count[p] > 0 ? s : NAN;
  else
    out[p] = src_count[p] > 0 ? s / (double)src_count[p] : NAN;
}

// ------------------------------------------------------------------------------------------
// two-directional Chamfer (cs_chamfer_2dir): both directions of a problem under ONE pose
// ------------------------------------------------------------------------------------------
// A work item is 256 ROWS of one direction of one problem, searched against all of that problem's COLUMNS: dir 0 = rows
// are posed sources, columns raw targets (k_chamfer's search); dir 1 = rows are raw targets, columns posed sources.  Either
// way the pair's value is the canonical d2 of (p_i, t_j): the differences of the two directions are exact negatives of each
// other and only their squares are used.  A row's minimum stays in its thread's register, so a column minimum of the
// problem is never combined across workgroups: no scratch per target row, no atomics, nothing shared between the problems
// of a call (DESIGN 18 sizes this against the one-pass form with a 64-bit atomicMin per column).  Columns are staged in
// LDS as f64 (dir 1: posed while staging), so the inner loop is three subtractions, a product, two fmas and a minimum.
struct Chamfer2Work {
  int64_t r0;   // first row of this tile (global row of d_src for dir 0, of d_tgt for dir 1)
  int64_t c0;   // first column (global row of the other array)
  int32_t rn;   // rows in this tile (<= 256)
  int32_t cn;   // columns
  int32_t prob;
  int32_t slot; // index into the partial-sum array
  int32_t dir;  // 0 forward, 1 backward
  int32_t pad;
};

__global__ __launch_bounds__(256) void k_chamfer2(const Chamfer2Work* __restrict__ work, const float* __restrict__ src,
                                                  const float* __restrict__ tgt, const float* __restrict__ T,
                                                  double* __restrict__ partial) {
  __shared__ double c_lds[CH_TT * 3];
  __shared__ double red[256];
  const Chamfer2Work wk = work[blockIdx.x];
  const int tid = threadIdx.x;
  const bool active = tid < wk.rn;
  const bool fwd = wk.dir == 0;
  const float* Tp = T + (int64_t)wk.prob * 16;
  const float* rows = fwd ? src : tgt;
  const float* cols = fwd ? tgt : src;
  double rx = 0, ry = 0, rz = 0;
  if (active) {
    const float* r = rows + (wk.r0 + tid) * 3;
    if (fwd) {
      chamfer_pose(Tp, r, &rx, &ry, &rz);
    } else {
      rx = r[0];
      ry = r[1];
      rz = r[2];
    }
  }
  double best = INFINITY;
  for (int cbase = 0; cbase < wk.cn; cbase += CH_TT) {
    const int ccount = min(CH_TT, wk.cn - cbase);
    __syncthreads();
    for (int j = tid; j < ccount; j += 256) {
      const float* c = cols + (wk.c0 + cbase + j) * 3;
      double cx, cy, cz;
      if (fwd) {
        cx = c[0];
        cy = c[1];
        cz = c[2];
      } else {
        chamfer_pose(Tp, c, &cx, &cy, &cz);
      }
      c_lds[3 * j + 0] = cx;
      c_lds[3 * j + 1] = cy;
      c_lds[3 * j + 2] = cz;
    }
    __syncthreads();
    if (!active) continue;
#pragma unroll 8
    for (int j = 0; j < ccount; ++j) {
      const double dx = rx - c_lds[3 * j + 0];
      const double dy = ry - c_lds[3 * j + 1];
      const double dz = rz - c_lds[3 * j + 2];
      const double d = fma(dz, dz, fma(dy, dy, dx * dx));
      // `best` is never NaN, so fmin is `d < best ? d : best` in one v_min_f64: a NaN d loses, +inf never replaces anything
      best = fmin(d, best);
    }
  }
  red[tid] = active ? sqrt(best) : 0.0;
  chamfer_block_reduce(red, tid, 0);
  if (tid == 0) partial[wk.slot] = red[0];
}

}  // namespace cs

using namespace cs;

// {tiles answered by the f16 ranking, of those recomputed by the f64 kernel}; counted only while CS_CHAMFER_STATS=1
// (the count costs a synchronisation)
static std::atomic<unsigned long long> g_chamfer_stats[2];

// The environment switches of cs_chamfer_1dir / cs_hausdorff_1dir.
struct ChamferOptions {
  enum Path { F16, F64, EXHAUSTIVE };
  // CS_CHAMFER_MFMA=0: the exhaustive all-VALU chain kernel; CS_CHAMFER_F16=0: the f64 matrix-pipe kernel for every
  // tile; default: the f16 matrix-core ranking, the f64 kernel only for the tiles it flags
  Path path;
  bool stats;  // CS_CHAMFER_STATS=1: count the tiles the f16 path handed to the f64 kernel (synchronises)
};
static ChamferOptions read_options() {
  ChamferOptions o;
  o.path = env_first_is("CS_CHAMFER_MFMA", '0')  ? ChamferOptions::EXHAUSTIVE
           : env_first_is("CS_CHAMFER_F16", '0') ? ChamferOptions::F64
                                                 : ChamferOptions::F16;
  o.stats = env_first_is("CS_CHAMFER_STATS", '1');
  return o;
}

// The nearest-target search of every work item: partial[w.slot] = sum (or max) of the tile's nearest distances.
// nt_rows: target rows the problems refer to, [0, nt_rows).
static int chamfer_rank(const ChamferOptions& opt, const ChamferWork* d_work, unsigned n_work, const float* d_src,
                        const float* d_tgt, int64_t nt_rows, const float* d_T, int reduce_max, double* partial,
                        hipStream_t s) {
  const dim3 grid(n_work);
  if (opt.path == ChamferOptions::EXHAUSTIVE) {
    hipLaunchKernelGGL(k_chamfer, grid, dim3(256), 0, s, d_work, d_src, d_tgt, d_T, reduce_max, partial);
    return CS_OK;
  }
  PoolBuf<double> t4g((size_t)(nt_rows ? nt_rows : 1) * 4);
  CS_REQUIRE(t4g.p, CS_ERR_HIP, "cs_chamfer_1dir: scratch allocation failed");
  if (nt_rows)
    hipLaunchKernelGGL(k_chamfer_pack, dim3((unsigned)ceil_div(nt_rows, 256)), dim3(256), 0, s, d_tgt, nt_rows, t4g.p);
  if (opt.path == ChamferOptions::F64) {
    hipLaunchKernelGGL(k_chamfer_mfma, grid, dim3(256), 0, s, d_work, d_src, d_tgt, t4g.p, d_T, reduce_max, partial,
                       (const int32_t*)nullptr);
    return CS_OK;
  }
  ChfImage im;
  PoolBuf<int32_t> wflag(n_work);
  CS_REQUIRE(wflag.p && im.pack(d_tgt, nt_rows, s), CS_ERR_HIP, "cs_chamfer_1dir: scratch allocation failed");
  hipLaunchKernelGGL(k_chamfer_f16, grid, dim3(256), 0, s, d_work, d_src, im.t4f.p, im.img16.p, im.tn16.p, d_T,
                     reduce_max, partial, wflag.p);
  hipLaunchKernelGGL(k_chamfer_mfma, grid, dim3(256), 0, s, d_work, d_src, d_tgt, t4g.p, d_T, reduce_max, partial,
                     wflag.p);
  if (opt.stats) {
    unsigned long long h = 0;
    const int rc = count_flagged(wflag.p, (int64_t)n_work, &h, s, "cs_chamfer_1dir");
    if (rc) return rc;
    g_chamfer_stats[0] += n_work;
    g_chamfer_stats[1] += h;
  }
  return CS_OK;
}

// What both drivers do once their work list stands: upload it with the slot table (slot_begin[o] .. slot_begin[o + 1] = the
// work items of output o) and the row counts, run `search(d_work, partial)` (it fills partial[w.slot] of every work item)
// and finish every output from its slots -- the mean or the maximum, NaN for an output without rows.
template <typename Work, typename Search>
static int chamfer_search_finish(const char* who, const char* family, double flop, const std::vector<Work>& work,
                                 const std::vector<int32_t>& slot_begin, const std::vector<int64_t>& count, int reduce_max,
                                 double* d_out, hipStream_t s, Search search) {
  const int n_out = (int)count.size();
  PoolBuf<Work> dwork;
  PoolBuf<int32_t> dslot;
  PoolBuf<int64_t> dcount;
  PoolBuf<double> partial(work.size() + 1);
  CS_REQUIRE(partial.p, CS_ERR_HIP, "%s: scratch allocation failed", who);
  int rc = upload(dwork, work, s);
  if (!rc) rc = upload(dslot, slot_begin, s);
  if (!rc) rc = upload(dcount, count, s);
  if (rc) return rc;
  ProfScope prof(family, s, flop);
  if (!work.empty()) {
    rc = search(dwork.p, partial.p);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_chamfer_finish, dim3((unsigned)ceil_div(n_out, 64)), dim3(64), 0, s, partial.p, dslot.p, dcount.p,
                     n_out, reduce_max, d_out);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

// Scratch goes back to this thread's stream-ordered cache when the call returns; outputs are valid in stream order.
static int nn_dist_reduce(const float* d_src, const int64_t* h_soff, const float* d_tgt,
                          const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg,
                          int n_prob, const float* d_T, int reduce_max, double* d_out, void* stream) {
  CS_REQUIRE(h_soff && h_toff && h_src_seg && h_tgt_seg && d_T && d_out, CS_ERR_INVALID,
             "cs_chamfer_1dir: NULL argument");
  if (n_prob <= 0) return CS_OK;
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const ChamferOptions opt = read_options();
  // work list: the matrix kernels take CHM_ST sources per workgroup, the exhaustive one a source per thread
  const int64_t stile = opt.path == ChamferOptions::EXHAUSTIVE ? 256 : CHM_ST;
  std::vector<ChamferWork> work;
  std::vector<int32_t> slot_begin(n_prob + 1, 0);
  std::vector<int64_t> src_count(n_prob, 0);
  int64_t nt_rows = 0;
  double ch_flop = 0.0;
  for (int p = 0; p < n_prob; ++p) {
    int ss = h_src_seg[p], ts = h_tgt_seg[p];
    CS_REQUIRE(ss >= 0 && ts >= 0, CS_ERR_INVALID, "cs_chamfer_1dir: negative segment id");
    int64_t sn = h_soff[ss + 1] - h_soff[ss], tn = h_toff[ts + 1] - h_toff[ts];
    CS_REQUIRE(sn >= 0 && tn >= 0 && tn < (1LL << 31), CS_ERR_INVALID,
               "cs_chamfer_1dir: bad segment in problem %d", p);
    slot_begin[p] = (int32_t)work.size();
    src_count[p] = sn;
    nt_rows = std::max<int64_t>(nt_rows, h_toff[ts + 1]);
    for (int64_t q = 0; q < sn; q += stile) {
      ChamferWork w;
      w.s0 = h_soff[ss] + q;
      w.t0 = h_toff[ts];
      w.sn = (int32_t)(sn - q < stile ? sn - q : stile);
      w.tn = (int32_t)tn;
      w.prob = p;
      w.slot = (int32_t)work.size();
      work.push_back(w);
      ch_flop += 8.0 * (double)w.sn * (double)w.tn;
    }
  }
  slot_begin[n_prob] = (int32_t)work.size();
  CS_REQUIRE(work.empty() || (d_src && d_tgt), CS_ERR_INVALID, "cs_chamfer_1dir: NULL point array");
  // per problem the mean (Chamfer) or the maximum (Hausdorff) of its tiles' partial results
  return chamfer_search_finish("cs_chamfer_1dir", "chamfer", ch_flop, work, slot_begin, src_count, reduce_max, d_out, s,
                               [&](const ChamferWork* d_work, double* partial) {
                                 return chamfer_rank(opt, d_work, (unsigned)work.size(), d_src, d_tgt, nt_rows, d_T,
                                                     reduce_max, partial, s);
                               });
}

// cs_chamfer_2dir: the work list holds, per problem, the forward tiles then the backward tiles; direction h = 2 p + dir is
// finished like a problem of cs_chamfer_1dir (k_chamfer_finish over 2 n_prob "half problems": tiles left to right, mean,
// NaN for a direction without rows), which writes d_out[2 p + dir].
static int chamfer_2dir(const float* d_src, const int64_t* h_soff, const float* d_tgt, const int64_t* h_toff,
                        const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob, const float* d_T, double* d_out,
                        void* stream) {
  CS_REQUIRE(h_soff && h_toff && h_src_seg && h_tgt_seg && d_T && d_out, CS_ERR_INVALID, "cs_chamfer_2dir: NULL argument");
  if (n_prob <= 0) return CS_OK;
  CS_REQUIRE(n_prob < (1 << 30), CS_ERR_INVALID, "cs_chamfer_2dir: too many problems");
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  std::vector<Chamfer2Work> work;
  std::vector<int32_t> slot_begin(2 * (size_t)n_prob + 1, 0);
  std::vector<int64_t> row_count(2 * (size_t)n_prob, 0);
  double ch_flop = 0.0;
  for (int p = 0; p < n_prob; ++p) {
    const int ss = h_src_seg[p], ts = h_tgt_seg[p];
    CS_REQUIRE(ss >= 0 && ts >= 0, CS_ERR_INVALID, "cs_chamfer_2dir: negative segment id");
    const int64_t sn = h_soff[ss + 1] - h_soff[ss], tn = h_toff[ts + 1] - h_toff[ts];
    CS_REQUIRE(sn >= 0 && tn >= 0 && sn < (1LL << 31) && tn < (1LL << 31) && h_soff[ss] >= 0 && h_toff[ts] >= 0,
               CS_ERR_INVALID, "cs_chamfer_2dir: bad segment in problem %d", p);
    for (int dir = 0; dir < 2; ++dir) {
      const int64_t rn = dir ? tn : sn, cn = dir ? sn : tn;
      slot_begin[2 * (size_t)p + dir] = (int32_t)work.size();
      row_count[2 * (size_t)p + dir] = rn;
      for (int64_t q = 0; q < rn; q += 256) {
        Chamfer2Work w;
        w.r0 = (dir ? h_toff[ts] : h_soff[ss]) + q;
        w.c0 = dir ? h_soff[ss] : h_toff[ts];
        w.rn = (int32_t)(rn - q < 256 ? rn - q : 256);
        w.cn = (int32_t)cn;
        w.prob = p;
        w.slot = (int32_t)work.size();
        w.dir = dir;
        w.pad = 0;
        CS_REQUIRE(work.size() < (size_t)0x7fffffff, CS_ERR_INVALID, "cs_chamfer_2dir: too many tiles");
        work.push_back(w);
        ch_flop += 8.0 * (double)w.rn * (double)w.cn;
      }
    }
  }
  slot_begin[2 * (size_t)n_prob] = (int32_t)work.size();
  CS_REQUIRE(work.empty() || (d_src && d_tgt), CS_ERR_INVALID, "cs_chamfer_2dir: NULL point array");
  return chamfer_search_finish("cs_chamfer_2dir", "chamfer2", ch_flop, work, slot_begin, row_count, 0, d_out, s,
                               [&](const Chamfer2Work* d_work, double* partial) {
                                 hipLaunchKernelGGL(k_chamfer2, dim3((unsigned)work.size()), dim3(256), 0, s, d_work, d_src,
                                                    d_tgt, d_T, partial);
                                 return CS_OK;
                               });
}

extern "C" {

int cs_chamfer_2dir(const float* d_src, const int64_t* h_soff, const float* d_tgt, const int64_t* h_toff,
                    const int32_t* h_src_seg, const int32_t* h_tgt_seg, int n_prob, const float* d_T, double* d_out,
                    void* stream) {
  return chamfer_2dir(d_src, h_soff, d_tgt, h_toff, h_src_seg, h_tgt_seg, n_prob, d_T, d_out, stream);
}

void cs_chamfer_f16_stats(uint64_t out[2], int reset) { read_stats(g_chamfer_stats, out, reset); }

int cs_chamfer_1dir(const float* d_src, const int64_t* h_soff, const float* d_tgt,
                    const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg,
                    int n_prob, const float* d_T, double* d_out, void* stream) {
  return nn_dist_reduce(d_src, h_soff, d_tgt, h_toff, h_src_seg, h_tgt_seg, n_prob, d_T, 0, d_out,
                        stream);
}

int cs_hausdorff_1dir(const float* d_src, const int64_t* h_soff, const float* d_tgt,
                      const int64_t* h_toff, const int32_t* h_src_seg, const int32_t* h_tgt_seg,
                      int n_prob, const float* d_T, double* d_out, void* stream) {
  return nn_dist_reduce(d_src, h_soff, d_tgt, h_toff, h_src_seg, h_tgt_seg, n_prob, d_T, 1, d_out,
                        stream);
}

}  // extern "C"
