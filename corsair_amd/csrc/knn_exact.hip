// The exhaustive feature k-NN kernel: every target row gets the canonical evaluation (knn.hip: the contract).  It is the
// whole of cs_knn_feat for 3-d, 32-d and 33-d (FPFH) features, k = 7 / 8 and CS_KNN_MFMA=0, the fallback of the f16 shortlist path
// (knn_f16.hip: flagged tiles only), and what the tests hold that path against.
#include "knn.h"

namespace cs {

constexpr int KNN_TT = 128;  // target rows per LDS tile

template <int DIM>
__global__ __launch_bounds__(256) void k_knn_feat(const KnnWork* __restrict__ work,
                                                  const float* __restrict__ qf,
                                                  const float* __restrict__ tf, int k,
                                                  const int32_t* __restrict__ qlabel,
                                                  const int32_t* __restrict__ tlabel,
                                                  const int32_t* __restrict__ perm,
                                                  int32_t* __restrict__ out_idx,
                                                  double* __restrict__ out_dist,
                                                  const int32_t* __restrict__ tile_flag,
                                                  const int32_t* __restrict__ qflag) {
  // fallback mode (k_knn_rescore_f16 flagged some queries): only flagged tiles run, only flagged
  // queries are written
  if (tile_flag && !tile_flag[blockIdx.x]) return;
  // targets are converted to f64 once per tile (the inner loop is f64-VALU bound: one v_cvt less
  // per dimension and pair)
  __shared__ double t_lds[KNN_TT * DIM];
  __shared__ int32_t tl_lds[KNN_TT];
  const KnnWork wk = work[blockIdx.x];
  const int tid = threadIdx.x;
  const bool active = tid < wk.qn;
  const int64_t qrow = wk.q0 + (active ? tid : 0);

  double q[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) q[c] = (double)qf[qrow * DIM + c];
  int want = -1;
  const bool use_labels = qlabel != nullptr;
  if (use_labels) {
    int ql = qlabel[qrow];
    want = (ql >= 0 && ql < 8) ? perm[wk.prob * 8 + ql] : -2;
  }

  double bd[KNN_MAXK];
  int32_t bi[KNN_MAXK];
#pragma unroll
  for (int j = 0; j < KNN_MAXK; ++j) {
    bd[j] = INFINITY;
    bi[j] = -1;
  }

  for (int tbase = 0; tbase < wk.tn; tbase += KNN_TT) {
    const int tcount = min(KNN_TT, wk.tn - tbase);
    __syncthreads();
    for (int i = tid; i < tcount * DIM; i += 256) t_lds[i] = (double)tf[(wk.t0 + tbase) * DIM + i];
    if (use_labels)
      for (int i = tid; i < tcount; i += 256) tl_lds[i] = tlabel[wk.t0 + tbase + i];
    __syncthreads();
    if (!active) continue;
    for (int j = 0; j < tcount; ++j) {
      if (use_labels && tl_lds[j] != want) continue;
      double d = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        double diff = q[c] - t_lds[j * DIM + c];
        d = fma(diff, diff, d);
      }
      if (d < bd[KNN_MAXK - 1]) {
        // insert (d, tbase + j) into the running top-8 (ascending); strict < keeps the earlier
        // index on ties.  The first k entries are the answer.
        double cd = d;
        int32_t ci = tbase + j;
        bool carry = false;  // once placed, the displaced tail shifts down unconditionally
#pragma unroll
        for (int s = 0; s < KNN_MAXK; ++s) {
          if (carry || cd < bd[s]) {
            carry = true;
            double td = bd[s];
            int32_t ti = bi[s];
            bd[s] = cd;
            bi[s] = ci;
            cd = td;
            ci = ti;
          }
        }
      }
    }
  }
  if (active && (!qflag || qflag[wk.o0 + tid])) {
    for (int j = 0; j < k; ++j) {
      // (unrolled select keeps bd/bi in registers)
      double dj = INFINITY;
      int32_t ij = -1;
#pragma unroll
      for (int s = 0; s < KNN_MAXK; ++s)
        if (s == j) {
          dj = bd[s];
          ij = bi[s];
        }
      const int64_t orow = wk.o0 + tid;
      out_idx[orow * k + j] = ij;
      if (out_dist) out_dist[orow * k + j] = ij >= 0 ? sqrt(dj) : INFINITY;
    }
  }
}

template <int DIM>
static void launch(const KnnCall& c, const int32_t* tile_flag, const int32_t* qflag) {
  hipLaunchKernelGGL((k_knn_feat<DIM>), dim3(c.n_work), dim3(256), 0, c.s, c.d_work, c.d_qf, c.d_tf, c.k, c.d_qlabel,
                     c.d_tlabel, c.d_perm, c.d_idx, c.d_dist, tile_flag, qflag);
}

void knn_exact_launch(const KnnCall& c, const int32_t* tile_flag, const int32_t* qflag) {
  if (c.dim == 16) launch<16>(c, tile_flag, qflag);
  else if (c.dim == 32) launch<32>(c, tile_flag, qflag);
  else if (c.dim == 33) launch<33>(c, tile_flag, qflag);
  else launch<3>(c, tile_flag, qflag);
}

}  // namespace cs
