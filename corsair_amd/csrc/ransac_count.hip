// RANSAC exact inlier counts, f64 (Open3D evaluates Matrix4d * Vector4d and squaredNorm in double); see ransac.hip for the
// round they belong to.  No matrix cores here: the chain is residual2_f64 (ransac.h), the oracle's.
//   k_ransac_count      every hypothesis of an unfiltered chunk (<false>), or a long survivor list (<true>)
//   k_ransac_count_few  the usual handful of survivors: count and fixed-point error in one pass
//   k_ransac_err        fixed-point squared error of the candidates k_ransac_scan1 listed
// k_ransac_count: grid x = (hypothesis tile of 256) * splits + split, y = problem; block = 256 lanes = 256 hypotheses.
// A lane keeps its hypothesis in 12 f64 registers and walks the pair range of its split; pairs are
// staged 256 at a time: each thread loads one pair (6 coalesced f32 loads from the SoA copy), converts
// it to f64 once and stores it as one 48-B LDS row, which all lanes then read as broadcasts.
#include <algorithm>

#include "ransac.h"

namespace cs {

// LIST: the hypotheses are the survivors of the prefilter, hlist[p][0 .. n_surv[p]) (any order).
// HPW = hypotheses per workgroup: 256 (one per lane) or 64 (round 5: the FIRST chunk of a call, 64 iterations counted
// exactly before there is a best count to prune against -- lane = hypothesis + 64 x quarter, every quarter (= wave) takes
// every fourth staged pair and the four partial counts meet in the integer atomics the pair-range splits use anyway).
template <bool LIST, int HPW>
__device__ __forceinline__ void ransac_count_tile(double (*lds)[RC_CHUNK][6], const int p, const int tile,
                                                  const int split,
                                                  const RansacProb* __restrict__ probs,
                                                  const float* __restrict__ pk, int64_t total,
                                                  const double* __restrict__ hyp, int it0,
                                                  int bcount, int bmax, int splits, double thr2,
                                                  int32_t* __restrict__ res_cnt,
                                                  const int32_t* __restrict__ hlist,
                                                  const int32_t* __restrict__ n_surv) {
  const RansacProb pr = probs[p];
  if (pr.done) return;
  static_assert(HPW == RC_HYP || (!LIST && HPW == 64), "hypotheses per workgroup");
  constexpr int NPART = RC_HYP / HPW;                     // lanes that share a hypothesis (pair-interleaved)
  const int nlist = LIST ? n_surv[p] : 0;
  if (LIST) {
    if (tile * HPW >= nlist) return;
  } else {
    if (it0 + tile * HPW >= pr.est_k || tile * HPW >= bcount) return;  // whole block beyond the bound
  }
  const int tid = threadIdx.x;
  const int part = tid / HPW;
  const int h = tile * HPW + (tid - part * HPW);          // hypothesis slot of this lane
  const bool mine = LIST ? h < nlist : (h < bcount && it0 + h < pr.est_k);
  const int hsel = LIST ? hlist[(int64_t)p * bmax + min(h, nlist - 1)] : min(h, bmax - 1);
  double R[12];
  {
    const double* hp = hyp + ((int64_t)p * 12) * bmax + hsel;
#pragma unroll
    for (int e = 0; e < 12; ++e) R[e] = hp[(int64_t)e * bmax];
  }
  const int per = ((pr.m + splits - 1) / splits + RC_CHUNK - 1) / RC_CHUNK * RC_CHUNK;
  const int beg = split * per;
  const int end = min(pr.m, beg + per);
  int cnt = 0;
  // staging registers: the next stage's pair of this thread is in flight while the current stage is
  // evaluated; rows past the range become far-away targets (never inliers)
  float stg[6];
  auto stage_load = [&](int base) {
    const int i = base + tid;
    const int64_t g = pr.off + (i < end ? i : 0);
#pragma unroll
    for (int c = 0; c < 6; ++c) stg[c] = pk[(int64_t)c * total + g];
  };
  auto stage_store = [&](int b, int base) {
    const bool ok = base + tid < end;
#pragma unroll
    for (int c = 0; c < 6; ++c) lds[b][tid][c] = ok ? (double)stg[c] : (c >= 3 ? 1.0e30 : 0.0);
  };
  if (beg < end) {
    stage_load(beg);
    stage_store(0, beg);
  }
  int buf = 0;
  for (int base = beg; base < end; base += RC_CHUNK) {
    __syncthreads();
    const bool more = base + RC_CHUNK < end;
    if (more) stage_load(base + RC_CHUNK);
    const int nrow = min(RC_CHUNK, end - base);
    if (nrow == RC_CHUNK) {
#pragma unroll 4
      for (int j = part; j < RC_CHUNK; j += NPART) {
        const double* q = lds[buf][j];
        cnt += residual2_f64(R, q[0], q[1], q[2], q[3], q[4], q[5]) < thr2 ? 1 : 0;
      }
    } else {
      for (int j = part; j < nrow; j += NPART) {
        const double* q = lds[buf][j];
        cnt += residual2_f64(R, q[0], q[1], q[2], q[3], q[4], q[5]) < thr2 ? 1 : 0;
      }
    }
    if (more) stage_store(buf ^ 1, base + RC_CHUNK);
    buf ^= 1;
  }
  if (mine) {
    if (splits == 1 && NPART == 1)
      res_cnt[(int64_t)p * bmax + hsel] = cnt;
    else
      atomicAdd(&res_cnt[(int64_t)p * bmax + hsel], cnt);   // (res_cnt of the chunk is zero on entry)
  }
}

// grid: x = (hypothesis tile of 256) * splits + split, y = problem.  LIST: the survivor count is only
// known on the device, so a fixed number of tile slots (gridDim.x / splits) strides over the list.
template <bool LIST, int HPW = RC_HYP>
__global__ __launch_bounds__(256) void k_ransac_count(const RansacProb* __restrict__ probs,
                                                      const float* __restrict__ pk, int64_t total,
                                                      const double* __restrict__ hyp, int it0,
                                                      int bcount, int bmax, int splits, double thr2,
                                                      int32_t* __restrict__ res_cnt,
                                                      const int32_t* __restrict__ hlist,
                                                      const int32_t* __restrict__ n_surv) {
  // [buf][j][c]: c = 0..2 source xyz, c = 3..5 target xyz of pair j, f64 (one 48-B row per pair)
  __shared__ __attribute__((aligned(16))) double lds[2][RC_CHUNK][6];
  const int p = blockIdx.y;
  const int tile0 = blockIdx.x / splits;
  const int split = blockIdx.x - tile0 * splits;
  if (LIST) {
    const int nlist = n_surv[p];
    const int tstride = gridDim.x / splits;
    for (int tile = tile0; tile * RC_HYP < nlist; tile += tstride) {
      ransac_count_tile<LIST, HPW>(lds, p, tile, split, probs, pk, total, hyp, it0, bcount, bmax, splits, thr2,
                                   res_cnt, hlist, n_surv);
      __syncthreads();  // the next tile restages LDS
    }
  } else {
    ransac_count_tile<LIST, HPW>(lds, p, tile0, split, probs, pk, total, hyp, it0, bcount, bmax, splits, thr2,
                                 res_cnt, hlist, n_surv);
  }
}

// Exact counts (and fixed-point errors) when only a handful of hypotheses survive the prefilter (the
// normal case: ~2 per problem and round).  The MFMA list kernel this replaced needed a 128-hypothesis tile per
// workgroup and cost ~110 us per round even for two survivors.  Here the pair range of a problem is
// split over gridDim.x workgroups, each walks its slice once per survivor with the canonical f64
// chain; integer partial sums are combined with atomics (exact, order-free).
// grid: x = pair slice, y = problem, z = survivor slot (strided).  res_cnt / err_by_h of the survivors
// are zero on entry.
__global__ __launch_bounds__(256) void k_ransac_count_few(const RansacProb* __restrict__ probs,
                                                          const float* __restrict__ pk, int64_t total,
                                                          const double* __restrict__ hyp, int bmax,
                                                          double thr2, double scale,
                                                          int32_t* __restrict__ res_cnt,
                                                          unsigned long long* __restrict__ err_by_h,
                                                          const int32_t* __restrict__ hlist,
                                                          const int32_t* __restrict__ n_surv, int list_stride,
                                                          // second stage (cnt2 != nullptr): entry c of the first-stage list is
                                                          // skipped when its K = 32 bound is below the best
                                                          const int32_t* __restrict__ cnt2) {
  const int p = blockIdx.y;
  const RansacProb pr = probs[p];
  if (pr.done) return;
  const int nlist = n_surv[p];
  // entries beyond the capacity of the compact list were not looked at by the second stage: they pass unfiltered
  auto next_entry = [&](int c) {
    if (cnt2)
      while (c < nlist && c < PF_S2_CAP && cnt2[(int64_t)p * PF_S2_CAP + c] < pr.best_cnt) c += gridDim.z;
    return c;
  };
  int c = next_entry(blockIdx.z);
  if (c >= nlist) return;
  const int tid = threadIdx.x;
  const int per = (pr.m + gridDim.x - 1) / gridDim.x;
  const int i0 = blockIdx.x * per, i1 = min(pr.m, i0 + per);
  if (i0 >= i1) return;
  // this thread's pairs stay in registers across the survivors (slices are short: m / gridDim.x / 256)
  constexpr int MAXP = 8;
  const bool in_regs = per <= 256 * MAXP;
  float ps[MAXP][6];
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < MAXP; ++j) {
      const int i = i0 + tid + 256 * j;
      const int64_t g = pr.off + (i < i1 ? i : i0);
#pragma unroll
      for (int c = 0; c < 6; ++c) ps[j][c] = pk[(int64_t)c * total + g];
      if (i >= i1) ps[j][3] = 1.0e30f;  // far-away target: never an inlier
    }
  }
  // the next survivor's hypothesis is requested before the current one is evaluated: list entry -> twelve strided f64
  // loads are two dependent trips to L2 (~2 us), as long as the 8 x 22 f64 operations per thread they feed
  int hn = hlist[(int64_t)p * list_stride + c];
  double Rn[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) Rn[e] = hyp[((int64_t)p * 12 + e) * bmax + hn];
  for (; c < nlist;) {
    const int h = hn;
    double R[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) R[e] = Rn[e];
    c = next_entry(c + gridDim.z);
    if (c < nlist) {
      hn = hlist[(int64_t)p * list_stride + c];
#pragma unroll
      for (int e = 0; e < 12; ++e) Rn[e] = hyp[((int64_t)p * 12 + e) * bmax + hn];
    }
    int cnt = 0;
    unsigned long long err = 0;  // fixed-point squared error of the inliers (exact integer sum, as k_ransac_err)
    auto one = [&](float sx, float sy, float sz, float qx, float qy, float qz) {
      const double d2 = residual2_f64(R, (double)sx, (double)sy, (double)sz, (double)qx, (double)qy, (double)qz);
      if (d2 < thr2) {
        ++cnt;
        err += (unsigned long long)(d2 * scale);
      }
    };
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < MAXP; ++j) one(ps[j][0], ps[j][1], ps[j][2], ps[j][3], ps[j][4], ps[j][5]);
    } else {
      for (int i = i0 + tid; i < i1; i += 256) {
        const int64_t g = pr.off + i;
        one(pk[0 * total + g], pk[1 * total + g], pk[2 * total + g], pk[3 * total + g], pk[4 * total + g],
            pk[5 * total + g]);
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      cnt += __shfl_xor(cnt, off);
      err += __shfl_xor(err, off);
    }
    if ((tid & 63) == 0 && cnt) {
      atomicAdd(&res_cnt[(int64_t)p * bmax + h], cnt);
      atomicAdd(&err_by_h[(int64_t)p * bmax + h], err);
    }
  }
}

// Fixed-point squared error of the candidate hypotheses: grid (slots, problems).
__global__ __launch_bounds__(256) void k_ransac_err(const RansacProb* __restrict__ probs,
                                                    const float* __restrict__ pk, int64_t total,
                                                    const double* __restrict__ hyp, int bmax,
                                                    const int32_t* __restrict__ cand, double thr2,
                                                    double scale,
                                                    unsigned long long* __restrict__ cand_err) {
  __shared__ unsigned long long red[256];
  const int p = blockIdx.y;
  const RansacProb pr = probs[p];
  const int tid = threadIdx.x;
  for (int c = blockIdx.x; c < pr.n_cand; c += gridDim.x) {
    const int h = cand[(int64_t)p * bmax + c];
    const double* hp = hyp + ((int64_t)p * 12) * bmax + h;
    double R[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) R[e] = hp[(int64_t)e * bmax];
    unsigned long long err = 0;
    for (int i = tid; i < pr.m; i += 256) {
      const int64_t g = pr.off + i;
      const double d2 = residual2_f64(R, (double)pk[0 * total + g], (double)pk[1 * total + g],
                                      (double)pk[2 * total + g], (double)pk[3 * total + g],
                                      (double)pk[4 * total + g], (double)pk[5 * total + g]);
      if (d2 < thr2) err += (unsigned long long)(d2 * scale);
    }
    red[tid] = err;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    if (tid == 0) cand_err[(int64_t)p * bmax + c] = red[0];
    __syncthreads();
  }
}

void ransac_launch_count_chunk(const RansacIn& in, const double* hyp, int it0, int b, int hpw, int tiles, int splits,
                               double thr2, int32_t* res_cnt, hipStream_t s) {
  const dim3 grid((unsigned)(tiles * splits), (unsigned)in.n_prob);
  const auto kernel = hpw == 64 ? k_ransac_count<false, 64> : k_ransac_count<false, RC_HYP>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, in.probs, in.pk, in.tot1, hyp, it0, b, BMAX, splits, thr2, res_cnt,
                     (const int32_t*)nullptr, (const int32_t*)nullptr);
}

void ransac_launch_count_list(const RansacIn& in, const double* hyp, int it0, int b, double thr2, int32_t* res_cnt,
                              const int32_t* hlist, const int32_t* n_surv, hipStream_t s) {
  // few hypotheses, so the pair range is split finely
  int lsplits = 16;
  while (lsplits > 1 && in.m_max / lsplits < RC_CHUNK) --lsplits;
  const int ltiles = std::min((b + RC_HYP - 1) / RC_HYP, 4);  // tile slots; the kernel strides over longer lists
  hipLaunchKernelGGL(k_ransac_count<true>, dim3((unsigned)(ltiles * lsplits), (unsigned)in.n_prob), dim3(256), 0, s, in.probs,
                     in.pk, in.tot1, hyp, it0, b, BMAX, lsplits, thr2, res_cnt, hlist, n_surv);
}

void ransac_launch_count_few(const RansacIn& in, const double* hyp, double thr2, double scale, int32_t* res_cnt,
                             unsigned long long* err_by_h, const int32_t* hlist, const int32_t* n_surv, int fslots,
                             const int32_t* cnt2, hipStream_t s) {
  // pair slices short enough for a thread to keep its pairs in registers across the survivors (8 per thread)
  int fslices = 8;
  while (fslices < 32 && in.m_max > fslices * 2048) fslices *= 2;
  hipLaunchKernelGGL(k_ransac_count_few, dim3((unsigned)fslices, (unsigned)in.n_prob, (unsigned)fslots), dim3(256), 0, s,
                     in.probs, in.pk, in.tot1, hyp, BMAX, thr2, scale, res_cnt, err_by_h, hlist, n_surv, BMAX, cnt2);
}

void ransac_launch_err(const RansacIn& in, const double* hyp, const int32_t* cand, double thr2, double scale,
                       unsigned long long* cand_err, hipStream_t s) {
  hipLaunchKernelGGL(k_ransac_err, dim3(8, (unsigned)in.n_prob), dim3(256), 0, s, in.probs, in.pk, in.tot1, hyp, BMAX, cand,
                     thr2, scale, cand_err);
}
}  // namespace cs
