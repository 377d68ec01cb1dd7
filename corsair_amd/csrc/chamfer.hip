// One-directional Chamfer and Hausdorff distances of posed clouds, exact in f64 so that the values equal those of the
// reference's SciPy routine:
//   cs_chamfer_1dir / cs_hausdorff_1dir <- apply_transform + KDTree 1-NN   (utils/preprocess.py:39-48,67-70)
// The canonical distance of a source p = R s + t to a target is the f64 fma chain over x, y, z; the result of a source is
// the minimum over the targets.  Every distance that enters a sum or maximum is that of the canonical chain; the fast
// paths only decide WHICH targets get the canonical evaluation:
//   * default: k_chamfer_f16 ranks by |t|^2 - 2 p.t on the f16 matrix cores, evaluates the rows of the two best tiles
//     with the canonical chain and vouches for the result against its error budget; workgroups it cannot vouch for are
//     recomputed by k_chamfer_mfma (flag array, no host decision).  CS_CHAMFER_STATS=1 counts those workgroups
//     (cs_chamfer_f16_stats; synchronises).
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


#include "nn_common.h"

namespace cs {

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
  if (active) {
    const float* s = src + (wk.s0 + tid) * 3;
    double x = s[0], y = s[1], z = s[2];
    // row-major 4x4: p = R x + t, evaluated as fma(r0,x, fma(r1,y, fma(r2,z, t)))
    px = fma((double)Tp[0], x, fma((double)Tp[1], y, fma((double)Tp[2], z, (double)Tp[3])));
    py = fma((double)Tp[4], x, fma((double)Tp[5], y, fma((double)Tp[6], z, (double)Tp[7])));
    pz = fma((double)Tp[8], x, fma((double)Tp[9], y, fma((double)Tp[10], z, (double)Tp[11])));
  }
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
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] = reduce_max ? fmax(red[tid], red[tid + off]) : red[tid] + red[tid + off];
    __syncthreads();
  }
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
    const float* sp = src + (wk.s0 + (sloc < wk.sn ? sloc : 0)) * 3;
    const double x = sp[0], y = sp[1], z = sp[2];
    px[g] = fma((double)Tp[0], x, fma((double)Tp[1], y, fma((double)Tp[2], z, (double)Tp[3])));
    py[g] = fma((double)Tp[4], x, fma((double)Tp[5], y, fma((double)Tp[6], z, (double)Tp[7])));
    pz[g] = fma((double)Tp[8], x, fma((double)Tp[9], y, fma((double)Tp[10], z, (double)Tp[11])));
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
  __syncthreads();
  for (int off = CHM_ST / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] = reduce_max ? fmax(red[tid], red[tid + off]) : red[tid] + red[tid + off];
    __syncthreads();
  }
  if (tid == 0) partial[wk.slot] = red[0];
}

// ------------------------------------------------------------------------------------------
// The same search on the f16 matrix cores (round 5).  The f64 matrix pipe of gfx950 is the vector unit's double-precision
// ALU (78.6 TF either way): k_chamfer_mfma sits at 0.23 of it with five VALU operations per result on top.  The ranking
// value |t|^2 - 2 p.t needs nine products when the coordinates are cut into f16 hi + lo (ph.th + ph.tl + pl.th): ONE
// v_mfma_f32_32x32x16_f16 per 32 targets x 32 sources with |t|^2 in the accumulator input, 16x the rate per pair.  It only
// RANKS: a lane (one source, 16 of a tile's 32 target rows) keeps the two best TILE minima and the third best value (eight
// v_min3 per tile, no index per value); at the end the rows of its two tiles are evaluated with the canonical f64 chain,
// and the result is vouched for when it lies below the third value minus the error budget of the approximation -- then no
// row outside the evaluated tiles can be nearer.  A workgroup with a source that fails the test is recomputed by
// k_chamfer_mfma (flag array, no host decision).  Coordinates are scaled by 2^9 before the cut so that the lo parts stay
// normal f16 numbers; |coordinate| >= 60 does not fit and takes the f64 kernel as well.  Results: the same canonical
// distances as the other two kernels (tests/test_gpu_post.py::test_chamfer_matches_oracle, all three paths).
// (CHF_PITCH, CHF_ROWS, CHF_NG, CHF_SCALE: nn_common.h -- the ICP's association kernel reads the same image)
static_assert(4 * 32 * CHF_NG == CHM_ST, "the f16 kernel and its f64 fallback share the work items");

// target image: row j = [th(3) | tl(3) | th(3) | 0(7) | pad(8)] of the scaled coordinates, tn32[j] = |S t|^2 (f64 chain,
// rounded to f32); rows [n, n_pad) are zero with tn32 = +inf (they never win)
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
  double px[CHF_NG], py[CHF_NG], pz[CHF_NG];
  f16x8 bop[CHF_NG];
  float b1[CHF_NG], b2[CHF_NG], b3[CHF_NG];
  int t1[CHF_NG], t2[CHF_NG];
  bool in_range = true;
#pragma unroll
  for (int g = 0; g < CHF_NG; ++g) {
    const int sloc = wave * 32 * CHF_NG + 32 * g + col;
    const float* sp = src + (wk.s0 + (sloc < wk.sn ? sloc : 0)) * 3;
    const double x = sp[0], y = sp[1], z = sp[2];
    px[g] = fma((double)Tp[0], x, fma((double)Tp[1], y, fma((double)Tp[2], z, (double)Tp[3])));
    py[g] = fma((double)Tp[4], x, fma((double)Tp[5], y, fma((double)Tp[6], z, (double)Tp[7])));
    pz[g] = fma((double)Tp[8], x, fma((double)Tp[9], y, fma((double)Tp[10], z, (double)Tp[11])));
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
  // register-staged double buffer: the next stage's 12 KiB image + |t|^2 are requested before this stage is computed
  const uint4* gimg = reinterpret_cast<const uint4*>(img + (int64_t)wk.t0 * CHF_PITCH);
  constexpr int U4_PER_STAGE = CHF_ROWS * CHF_PITCH * 2 / 16;   // 768 = 3 per thread
  uint4 st0, st1, st2;     // (three named registers: an array captured by the lambdas below went to scratch)
  float stn;
  float tmax2 = 0.0f;
  auto load_stage = [&](int base) {
    const uint4* g = gimg + (int64_t)base * (CHF_PITCH * 2 / 16) + tid;
    st0 = g[0];
    st1 = g[256];
    st2 = g[512];
    const int r = base + tid;
    stn = r < wk.tn ? tn32[wk.t0 + r] : INFINITY;   // rows past the segment (another problem's rows) never win
    if (r < wk.tn) tmax2 = fmaxf(tmax2, stn);
  };
  auto store_stage = [&](int b) {
    uint4* d = reinterpret_cast<uint4*>(a_s[b]) + tid;
    d[0] = st0;
    d[256] = st1;
    d[512] = st2;
    tn_s[b][tid] = stn;
  };
  static_assert(U4_PER_STAGE == 3 * 256, "three 16-byte pieces per thread");
  if (wk.tn > 0) {
    load_stage(0);
    store_stage(0);
  }
  int buf = 0;
  for (int base = 0; base < wk.tn; base += CHF_ROWS) {
    __syncthreads();
    const bool more = base + CHF_ROWS < wk.tn;
    if (more) load_stage(base + CHF_ROWS);
#pragma unroll 1
    for (int t = 0; t < CHF_ROWS / 32; ++t) {
      if (base + 32 * t >= wk.tn) break;   // whole tile past the range (block-uniform)
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
        // sorted insertion of the tile minimum without a branch: new j-th value = median of (old j-1-th, old j-th, m);
        // the tile ids follow the two comparisons
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
  // largest |S t|^2 of the segment (error budget)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) tmax2 = fmaxf(tmax2, __shfl_xor(tmax2, off));
  if (lane == 0) wmax[wave] = tmax2;
  __syncthreads();
  const double tmax = sqrt((double)fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))) / (double)CHF_SCALE;
  bool bad = !in_range || !(tmax < 60.0);
  const float4* trow = t4f + wk.t0;
  auto eval_tile = [&](int g, int tile) {   // canonical distances of this lane's 16 rows of a tile: smallest
    double e = INFINITY;
    if (tile >= 0) {
      float4 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = tile * 32 + 4 * half + (i & 3) + 8 * (i >> 2);
        v[i] = trow[row < wk.tn ? row : 0];
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = tile * 32 + 4 * half + (i & 3) + 8 * (i >> 2);
        const double dx = px[g] - (double)v[i].x, dy = py[g] - (double)v[i].y, dz = pz[g] - (double)v[i].z;
        const double d = fma(dz, dz, fma(dy, dy, dx * dx));
        e = row < wk.tn ? fmin(e, d) : e;
      }
    }
    return e;
  };
#pragma unroll
  for (int g = 0; g < CHF_NG; ++g) {
    // Every unevaluated row has an approximate value >= the smallest tile minimum that was not evaluated (in scaled units
    // S^2 (|t|^2 - 2 p.t)), hence an exact one >= that - eps with eps covering: <= 16 f32 accumulation steps relative to
    // sum |terms| <= (|P| + |T|)^2, the dropped lo.lo products and the hi + lo cut residuals (2^-22 relative each), the f32
    // rounding of |T|^2 -- together < 2^-20 (|P| + |T|max)^2, charged 2^-19 -- and lo parts below the f16 normal range
    // should the matrix pipe flush them (<= 2^-14 per product side: 2^-10 (|P| + |T|max) covers all nine).
    const double pn2 = fma(pz[g], pz[g], fma(py[g], py[g], px[g] * px[g]));
    const double S = (double)CHF_SCALE, PT = S * (sqrt(pn2) + tmax);
    const double eps = 0x1.0p-19 * PT * PT + 0x1.0p-10 * PT;
    // best tile of either lane of the source first; the second tiles only where that does not settle it
    double e = eval_tile(g, t1[g]);
    e = fmin(e, __shfl_xor(e, 32));
    float rest = fminf(b2[g], __shfl_xor(b2[g], 32));     // smallest unevaluated tile minimum of the source
    bool ok = rest == INFINITY || (e - pn2) * S * S <= (double)rest - eps;
    if (__any(!ok)) {
      double e2 = ok ? INFINITY : eval_tile(g, t2[g]);
      e2 = fmin(e2, __shfl_xor(e2, 32));
      if (!ok) {
        e = fmin(e, e2);
        rest = fminf(b3[g], __shfl_xor(b3[g], 32));
        ok = rest == INFINITY || (e - pn2) * S * S <= (double)rest - eps;
      }
    }
    const int sloc = wave * 32 * CHF_NG + 32 * g + col;
    if (sloc < wk.sn && !ok) bad = true;
    if (half == 0) red[sloc] = sloc < wk.sn ? sqrt(e) : 0.0;
  }
  if (__any(bad) && lane == 0) atomicOr(&wg_bad, 1);
  __syncthreads();
  for (int off = CHM_ST / 2; off > 0; off >>= 1) {
    if (tid < off) red[tid] = reduce_max ? fmax(red[tid], red[tid + off]) : red[tid] + red[tid + off];
    __syncthreads();
  }
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

__device__ __forceinline__ void chamfer_pose(const float* __restrict__ Tp, const float* __restrict__ s, double* px,
                                             double* py, double* pz) {
  const double x = s[0], y = s[1], z = s[2];
  // row-major 4x4: p = R x + t, evaluated as fma(r0,x, fma(r1,y, fma(r2,z, t))) -- k_chamfer's chain
  *px = fma((double)Tp[0], x, fma((double)Tp[1], y, fma((double)Tp[2], z, (double)Tp[3])));
  *py = fma((double)Tp[4], x, fma((double)Tp[5], y, fma((double)Tp[6], z, (double)Tp[7])));
  *pz = fma((double)Tp[8], x, fma((double)Tp[9], y, fma((double)Tp[10], z, (double)Tp[11])));
}

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
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] = red[tid] + red[tid + off];
    __syncthreads();
  }
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
  // image rows padded by one stage: the last stage of the last segment reads past its end
  const int64_t n_pad = nt_rows + CHF_ROWS;
  PoolBuf<_Float16> img16((size_t)n_pad * CHF_PITCH);
  PoolBuf<float> tn16((size_t)n_pad);
  PoolBuf<float4> t4f((size_t)(nt_rows ? nt_rows : 1));
  PoolBuf<int32_t> wflag(n_work);
  CS_REQUIRE(img16.p && tn16.p && wflag.p && t4f.p, CS_ERR_HIP, "cs_chamfer_1dir: scratch allocation failed");
  chamfer_pack16(d_tgt, nt_rows, n_pad, img16.p, tn16.p, t4f.p, s);
  hipLaunchKernelGGL(k_chamfer_f16, grid, dim3(256), 0, s, d_work, d_src, t4f.p, img16.p, tn16.p, d_T, reduce_max,
                     partial, wflag.p);
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
  PoolBuf<ChamferWork> dwork;
  PoolBuf<int32_t> dslot;
  PoolBuf<int64_t> dcount;
  PoolBuf<double> partial(work.size() + 1);
  CS_REQUIRE(partial.p, CS_ERR_HIP, "cs_chamfer_1dir: scratch allocation failed");
  int rc = upload(dwork, work, s);
  if (!rc) rc = upload(dslot, slot_begin, s);
  if (!rc) rc = upload(dcount, src_count, s);
  if (rc) return rc;
  ProfScope prof("chamfer", s, ch_flop);
  if (!work.empty()) {
    rc = chamfer_rank(opt, dwork.p, (unsigned)work.size(), d_src, d_tgt, nt_rows, d_T, reduce_max, partial.p, s);
    if (rc) return rc;
  }
  // finish: per problem the mean (Chamfer) or the maximum (Hausdorff) of its tiles' partial results
  hipLaunchKernelGGL(k_chamfer_finish, dim3((unsigned)ceil_div(n_prob, 64)), dim3(64), 0, s,
                     partial.p, dslot.p, dcount.p, n_prob, reduce_max, d_out);
  CS_LAUNCH_CHECK();
  return CS_OK;
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
  PoolBuf<Chamfer2Work> dwork;
  PoolBuf<int32_t> dslot;
  PoolBuf<int64_t> dcount;
  PoolBuf<double> partial(work.size() + 1);
  CS_REQUIRE(partial.p, CS_ERR_HIP, "cs_chamfer_2dir: scratch allocation failed");
  int rc = upload(dwork, work, s);
  if (!rc) rc = upload(dslot, slot_begin, s);
  if (!rc) rc = upload(dcount, row_count, s);
  if (rc) return rc;
  ProfScope prof("chamfer2", s, ch_flop);
  if (!work.empty())
    hipLaunchKernelGGL(k_chamfer2, dim3((unsigned)work.size()), dim3(256), 0, s, dwork.p, d_src, d_tgt, d_T, partial.p);
  hipLaunchKernelGGL(k_chamfer_finish, dim3((unsigned)ceil_div(2 * (int64_t)n_prob, 64)), dim3(64), 0, s, partial.p,
                     dslot.p, dcount.p, 2 * n_prob, 0, d_out);
  CS_LAUNCH_CHECK();
  return CS_OK;
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
