// The f16 matrix-core ranking scan of 3-d points that k_chamfer_f16 (chamfer.hip) and k_icp_f16 (icp_assoc.hip) share, and
// nothing else: the target image and its host-side preparation, the lane's ranking state, the operand of a posed source, the
// scan of a target segment, the error budget, and the canonical evaluation of the rows of a tile.  The kernels differ only in
// what they do with the evaluated rows (a minimum, or a (distance, row) pair) and in how strictly they vouch for them.
//   value v~ = f32(|S t|^2) + the nine products th.(-2 ph) + tl.(-2 ph) + th.(-2 pl) of the coordinates scaled by S =
//   CHF_SCALE and cut into f16 hi + lo, accumulated in f32 by ONE v_mfma_f32_32x32x16_f16 per 32 targets x 32 sources,
//   stands for S^2 (|t|^2 - 2 p.t) = S^2 (d - |p|^2).
//   rows = targets (LDS, staged through registers from the 48-B-pitch image), cols = posed sources (registers): a lane owns
//   one source of each of its wave's CHF_NG groups and 16 of a tile's 32 target rows; the two lanes of a source (lane,
//   lane ^ 32) own disjoint halves.
// It only RANKS: a lane keeps the two best TILE minima with their tile ids and the third best value (eight v_min3 per tile,
// no index per value).  The kernel then evaluates the rows of those tiles with the canonical f64 chain and vouches for the
// result when it lies below the smallest tile minimum that was not evaluated minus chf_eps: no row outside the evaluated
// tiles can then be nearer.
#pragma once
#include "nn_common.h"

namespace cs {

// The image of the target rows: row j = [th(3) | tl(3) | th(3) | 0(7) | pad(8)] of the coordinates scaled by CHF_SCALE (the lo
// parts stay normal f16 numbers; |coordinate| >= 60 does not fit and is never vouched for), tn32[j] = |S t|^2 (f64 chain,
// rounded to f32), t4f[j] = (x, y, z, 0): the canonical evaluation reads a candidate row with one 16-byte request.
constexpr int CHF_PITCH = 24;     // halfs per image row (48 B: conflict-free ds_read_b128 fragments)
constexpr int CHF_ROWS = 256;     // target rows per LDS stage (8 MFMA row tiles)
constexpr int CHF_NG = 2;         // 32-source groups per wave
constexpr float CHF_SCALE = 512.0f;
// k_chamfer_pack16 (chamfer.hip) over rows [0, n_pad): rows [n, n_pad) are zero with tn32 = +inf.  Launch only.
void chamfer_pack16(const float* d_tgt, int64_t n, int64_t n_pad, _Float16* img, float* tn32, float4* t4f, hipStream_t s);

// The image of target rows [0, nt_rows) as a call owns it.  The image rows are padded by one stage: the scan loads whole
// stages, so the last stage of the last segment reads past its end (rows past a segment never win: chf_scan).
struct ChfImage {
  PoolBuf<_Float16> img16;
  PoolBuf<float> tn16;
  PoolBuf<float4> t4f;
  // allocates and enqueues the packing; false: an allocation failed
  bool pack(const float* d_tgt, int64_t nt_rows, hipStream_t s) {
    const int64_t n_pad = nt_rows + CHF_ROWS;
    if (!img16.alloc((size_t)n_pad * CHF_PITCH) || !tn16.alloc((size_t)n_pad) || !t4f.alloc((size_t)nt_rows)) return false;
    chamfer_pack16(d_tgt, nt_rows, n_pad, img16.p, tn16.p, t4f.p, s);
    return true;
  }
};

// What a lane carries through the scan, per group g of its wave: the posed source (the kernel's own pose chain fills it), its
// B operand, the three smallest tile minima b1 <= b2 <= b3 and the tiles of the first two (-1: none).
struct ChfRank {
  double px[CHF_NG], py[CHF_NG], pz[CHF_NG];
  f16x8 bop[CHF_NG];
  float b1[CHF_NG], b2[CHF_NG], b3[CHF_NG];
  int t1[CHF_NG], t2[CHF_NG];
  bool in_range = true;   // every source of the lane is finite and inside the f16 range
};

// The operand of group g from its posed coordinates: the hi / lo cut of -2 S p, the lane's half of the 16 k-rows, the
// range test, and the empty list.
__device__ __forceinline__ void chf_operand(ChfRank& r, int g, int half) {
  const float pf[3] = {(float)r.px[g] * CHF_SCALE, (float)r.py[g] * CHF_SCALE, (float)r.pz[g] * CHF_SCALE};
  _Float16 hi[3], lo[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    knf_split(-2.0f * pf[c], &hi[c], &lo[c]);
    r.in_range = r.in_range && fabsf(pf[c]) < 60.0f * CHF_SCALE;   // (NaN fails too)
  }
  // B rows k: 0..2 = -2 ph (x th), 3..5 = -2 ph (x tl), 6..8 = -2 pl (x th), 9..15 = 0; this lane holds k = 8 half .. + 7
  const _Float16 z0 = (_Float16)0.0f;
  if (half == 0)
    r.bop[g] = f16x8{hi[0], hi[1], hi[2], hi[0], hi[1], hi[2], lo[0], lo[1]};
  else
    r.bop[g] = f16x8{lo[2], z0, z0, z0, z0, z0, z0, z0};
  r.b1[g] = r.b2[g] = r.b3[g] = INFINITY;
  r.t1[g] = r.t2[g] = -1;
}

// The scan of the segment of tn target rows that starts at row t0 of the image: every lane's list afterwards ranks the
// segment's 32-row tiles (tile = row / 32 within the segment) for its sources.  Returns tmax, the largest |t| of the segment
// (error budget; a NaN row does not enter it, an infinite one makes it infinite).
// It contains barriers: all 256 threads of the workgroup call it, under block-uniform control flow.  a_s, tn_s and wmax are
// the caller's LDS; they are free again after the call.
__device__ __forceinline__ double chf_scan(ChfRank& r, const _Float16* __restrict__ img, const float* __restrict__ tn32,
                                           int64_t t0, int tn, _Float16 (&a_s)[2][CHF_ROWS * CHF_PITCH],
                                           float (&tn_s)[2][CHF_ROWS], float (&wmax)[4], int tid) {
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int half = lane >> 5;
  const int col = lane & 31;
  // register-staged double buffer: the next stage's 12 KiB image + |t|^2 are requested before this stage is computed
  const uint4* gimg = reinterpret_cast<const uint4*>(img + t0 * CHF_PITCH);
  constexpr int U4_PER_STAGE = CHF_ROWS * CHF_PITCH * 2 / 16;   // 768 = 3 per thread
  uint4 st0, st1, st2;     // (three named registers: an array captured by the lambdas below went to scratch)
  float stn;
  float tmax2 = 0.0f;
  auto load_stage = [&](int base) {
    const uint4* g = gimg + (int64_t)base * (CHF_PITCH * 2 / 16) + tid;
    st0 = g[0];
    st1 = g[256];
    st2 = g[512];
    const int row = base + tid;
    stn = row < tn ? tn32[t0 + row] : INFINITY;   // rows past the segment (another problem's rows) never win
    if (row < tn) tmax2 = fmaxf(tmax2, stn);
  };
  auto store_stage = [&](int b) {
    uint4* d = reinterpret_cast<uint4*>(a_s[b]) + tid;
    d[0] = st0;
    d[256] = st1;
    d[512] = st2;
    tn_s[b][tid] = stn;
  };
  static_assert(U4_PER_STAGE == 3 * 256, "three 16-byte pieces per thread");
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
        const f32x16 d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, r.bop[g], c16, 0, 0, 0);
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
        const float o1 = r.b1[g], o2 = r.b2[g];
        const bool lt1 = m < o1, lt2 = m < o2;
        r.b1[g] = fminf(o1, m);
        r.b2[g] = __builtin_amdgcn_fmed3f(o1, o2, m);
        r.b3[g] = __builtin_amdgcn_fmed3f(o2, r.b3[g], m);
        r.t2[g] = lt1 ? r.t1[g] : (lt2 ? tile : r.t2[g]);
        r.t1[g] = lt1 ? tile : r.t1[g];
      }
    }
    if (more) store_stage(buf ^ 1);
    buf ^= 1;
  }
  // largest |S t|^2 of the segment
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) tmax2 = fmaxf(tmax2, __shfl_xor(tmax2, off));
  if (lane == 0) wmax[wave] = tmax2;
  __syncthreads();
  return sqrt((double)fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]))) / (double)CHF_SCALE;
}

// The error budget of a source with |p|^2 = pn2 against a segment with largest |t| = tmax, in the scaled units of the ranking
// value.  Every unevaluated row has an approximate value >= the smallest tile minimum that was not evaluated (in scaled units
// S^2 (|t|^2 - 2 p.t)), hence an exact one >= that - eps with eps covering: <= 16 f32 accumulation steps relative to
// sum |terms| <= (|P| + |T|)^2, the dropped lo.lo products and the hi + lo cut residuals (2^-22 relative each), the f32
// rounding of |T|^2 -- together < 2^-20 (|P| + |T|max)^2, charged 2^-19 -- and lo parts below the f16 normal range
// should the matrix pipe flush them (<= 2^-14 per product side: 2^-10 (|P| + |T|max) covers all nine).
// A canonical d^2 = e of the source compares as (e - pn2) * S^2 against (tile minimum) - eps.  The budget holds for sources
// with in_range and tmax < 60.
__device__ __forceinline__ double chf_eps(double pn2, double tmax) {
  const double PT = (double)CHF_SCALE * (sqrt(pn2) + tmax);
  return 0x1.0p-19 * PT * PT + 0x1.0p-10 * PT;
}

// segment row of result element i (0..15) of a tile for the lanes of `half`: the row id of the MFMA result d[i]
__device__ __forceinline__ int chf_row(int tile, int half, int i) { return tile * 32 + 4 * half + (i & 3) + 8 * (i >> 2); }

// Canonical distances (the f64 fma chain over x, y, z) of the posed source (px, py, pz) to this lane's 16 rows of a tile of
// the segment whose float4 rows start at trow, rows ascending with a strict <: the smallest by (distance, row) in (e, er);
// (+inf, 0x7fffffff) for tile < 0, or when no row of the lane lies inside the segment at finite distance (a NaN loses).
__device__ __forceinline__ void chf_eval_tile(const float4* __restrict__ trow, int tn, int tile, int half, double px,
                                              double py, double pz, double& e, int& er) {
  e = INFINITY;
  er = 0x7fffffff;
  if (tile >= 0) {
    float4 v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = chf_row(tile, half, i);
      v[i] = trow[row < tn ? row : 0];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int row = chf_row(tile, half, i);
      const double dx = px - (double)v[i].x, dy = py - (double)v[i].y, dz = pz - (double)v[i].z;
      const double d = fma(dz, dz, fma(dy, dy, dx * dx));
      if (row < tn && d < e) {
        e = d;
        er = row;
      }
    }
  }
}

}  // namespace cs
