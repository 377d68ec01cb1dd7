// Feature k-NN of the registration path, exact in f64 so that the returned indices equal those of the reference's
// SciPy routine:
//   cs_knn_feat <- KDTree(feat1).query(feat0, k)     (utils/find_nn.py:43-49, utils/eval_pose.py:48-79,
//                                                     utils/symmetry.py:145-179)
// The canonical distance is one f64 fma chain over the feature dimension in ascending order, sum_c (q_c - t_c)^2;
// ties go to the smaller row.  Every returned index / distance is that of the canonical chain.  The fast paths only
// decide WHICH rows get the canonical evaluation:
//   * default (16-d features, k <= 6): k_knn_f16<1> bounds every query's k-th distance from tile minima, k_knn_f16<0>
//     shortlists by |t|^2 - 2 q.t on the f16 matrix cores, k_knn_rescore_f16 evaluates the shortlist with the canonical
//     chain, ranks it and VERIFIES it against the shortlist threshold; the queries that fail are recomputed by
//     k_knn_feat<16> (flagged tiles only).  CS_KNN_TWOPASS=0 drops the threshold pass; CS_KNN_STATS=1 counts the
//     recomputed queries (cs_knn_shortlist_stats; synchronises).
//   * CS_KNN_MFMA=64: k_knn_mfma16 shortlists on the f64 matrix pipe, k_knn_rescore16 ranks the shortlist with the
//     canonical chain; queries with |q|^2 >= KNF_RANGE (or not finite) are recomputed by k_knn_feat<16>.
// Non-finite rows (include/corsair_hip.h): a candidate whose canonical distance is NaN or +inf is never a neighbour.  Every
// insertion test is a strict `<` against a list that starts at +inf, the tile minima are fminf / v_min3 (a NaN operand
// loses), and the budgets take their maxima with fmaxf (a NaN row does not enter seg_t2max; an infinite or huge one
// makes it +inf, which sends the whole segment to the exhaustive kernel).
//   * CS_KNN_MFMA=0, and every other shape (3-d, 32-d, k = 7 / 8): k_knn_feat<DIM>, exhaustive on the VALU -- the fallback
//     of the f16 path and what the tests hold the other two against.
// Labelled searches (part-to-part correspondences): both shortlist paths visit the targets of a segment in label order
// (label_order: k_seg_keys, a radix sort, k_label_starts) and scan only the rows of the labels a workgroup wants.
// k_count_flags lives here; chamfer.hip reaches it through count_flagged().
#include <hipcub/hipcub.hpp>


#include "nn_common.h"

namespace cs {

// ------------------------------------------------------------------------------------------
// feature k-NN
// ------------------------------------------------------------------------------------------
struct KnnWork {
  int64_t q0;   // first query row of the tile (row of d_qf)
  int64_t t0;   // first target row of the problem (row of d_tf)
  int64_t o0;   // first output row of the tile (problem-major)
  int32_t qn;   // query rows in this tile (<= 256)
  int32_t tn;   // target rows
  int32_t prob;
  int32_t pad;
};

constexpr int KNN_MAXK = 8;
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

// ------------------------------------------------------------------------------------------
// feature k-NN on the f64 matrix pipe (16-d features, the registration path's shape).
// dist(q, t) = |q|^2 + |t|^2 - 2 q.t with the dot products on v_mfma_f64_16x16x4_f64: the VALU is left
// with 3 f64 ops per pair instead of 32.  The expansion rounds differently from the canonical chain,
// so it only SHORTLISTS: every lane keeps the KNM_KK best rows of its quarter of the targets by the
// expanded distance, k_knn_rescore re-evaluates the 4 x KNM_KK candidates of a query with the
// canonical chain sum_c (q_c - t_c)^2 and ranks them by (distance, row).  The result equals the exact
// kernel's unless more than KNM_KK - k rows of one quarter tie with the k-th neighbour to within the
// rounding of the expansion (~1e-15 relative) -- the caveat every f64 distance-matrix method has.
// Labelled searches (part-to-part correspondences): the targets of a segment are visited in label
// order (stable), so a wave skips the 16-row tiles whose labels cannot match its 16 queries.
// ------------------------------------------------------------------------------------------
constexpr int KNM_NG = 1;               // 16-query groups per wave (each A fragment is used NG times)
constexpr int KNM_QT = 64 * KNM_NG;     // queries per workgroup
constexpr int KNM_TT = 256;             // target rows per LDS stage (one row per thread)
constexpr int KNM_PITCH = 18;           // floats per LDS row: conflict-free ds_read_b32 of the A fragments
constexpr int KNM_KK = 8;               // shortlist per lane (k <= KNM_KK - 2)
constexpr int KNM_PEND = 4;             // pending (not yet ranked) candidates per lane

__global__ void k_seg_keys(const int64_t* __restrict__ off, int n_seg, const int32_t* __restrict__ label,
                           uint32_t* __restrict__ keys, int32_t* __restrict__ rows) {
  const int sg = blockIdx.y;
  const int64_t b = off[sg], e = off[sg + 1];
  for (int64_t i = b + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < e; i += (int64_t)gridDim.x * blockDim.x) {
    const int l = label[i];
    keys[i] = (uint32_t)sg * 16u + (uint32_t)((l >= 0 && l < 8) ? l : 8);
    rows[i] = (int32_t)(i - b);  // row local to the segment
  }
}

// lab_start[seg * 10 + l] = first row (label order, local to the segment) whose label key is >= l,
// l = 0..9 (keys: 0..7 parts, 8 = no part); one thread per entry, binary search in the sorted keys
__global__ void k_label_starts(const int64_t* __restrict__ off, int n_seg,
                               const uint32_t* __restrict__ keys_sorted, int32_t* __restrict__ lab_start) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_seg * 10) return;
  const int sg = i / 10, l = i - sg * 10;
  const int64_t b = off[sg], e = off[sg + 1];
  const uint32_t key = (uint32_t)sg * 16u + (uint32_t)l;
  int64_t lo = b, hi = e;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys_sorted[mid] < key) lo = mid + 1; else hi = mid;
  }
  lab_start[i] = (int32_t)(lo - b);
}

__global__ __launch_bounds__(256) void k_knn_mfma16(const KnnWork* __restrict__ work,
                                                    const float* __restrict__ qf,
                                                    const float* __restrict__ tf,
                                                    const double* __restrict__ qnorm,
                                                    const double* __restrict__ tnorm,
                                                    const int32_t* __restrict__ qlabel,
                                                    const int32_t* __restrict__ tlabel,
                                                    const int32_t* __restrict__ perm,
                                                    const int32_t* __restrict__ torder,
                                                    const int32_t* __restrict__ lab_start,
                                                    int32_t* __restrict__ cand_i) {
  // double-buffered stage: features (f32, converted when the fragment is read), |t|^2, label, row id
  __shared__ float t_lds[2][KNM_TT * KNM_PITCH];
  __shared__ double tn_lds[2][KNM_TT];
  __shared__ int32_t tl_lds[2][KNM_TT];
  __shared__ int32_t ti_lds[2][KNM_TT];
  __shared__ int32_t wrange[2][4];
  const KnnWork wk = work[blockIdx.x];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15;  // query within a group (B side); target row within a 16-row tile (A side)
  const int kq = lane >> 4;   // k slot of the operands; row group of the results
  const bool use_labels = qlabel != nullptr;
  double qb[KNM_NG][4], my_qn[KNM_NG];
  int want[KNM_NG];
  bool qvalid[KNM_NG];
  int wmin = 0x7fffffff, wmax = -2;
#pragma unroll
  for (int g = 0; g < KNM_NG; ++g) {
    const int qloc = wave * 16 * KNM_NG + 16 * g + col;
    qvalid[g] = qloc < wk.qn;
    const int64_t qrow = wk.q0 + (qvalid[g] ? qloc : 0);
#pragma unroll
    // B[k = 4 s + kq][query], pre-scaled by -2 (exact): with the accumulator preloaded with |t|^2 the
    // chain delivers |t|^2 - 2 q.t, the ranking value of the query (|q|^2 is the same for all targets)
    for (int s4 = 0; s4 < 4; ++s4) qb[g][s4] = -2.0 * (double)qf[qrow * 16 + 4 * s4 + kq];
    my_qn[g] = 0.0;
    want[g] = -1;
    if (use_labels) {
      const int ql = qlabel[qrow];
      want[g] = (qvalid[g] && ql >= 0 && ql < 8) ? perm[wk.prob * 8 + ql] : -2;
      if (want[g] >= 0) wmin = min(wmin, want[g]);
      wmax = max(wmax, want[g]);
    }
  }
  // label window of the wave's queries (tile skipping)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    wmin = min(wmin, __shfl_xor(wmin, off));
    wmax = max(wmax, __shfl_xor(wmax, off));
  }
  // Ranked shortlist (ascending) plus a small unranked pending list per lane.  A candidate below the
  // lane's threshold is only appended (a register shift); the pending lists of the whole wave are
  // ranked together when one of them is full.  Ranking on every hit would run the 8-slot insertion
  // for nearly every element, because some lane of the 64 almost always has a hit.
  // Labelled search: targets are visited in label order, and the queries of a workgroup (sorted by
  // part) want only one or two labels: the scan covers just the target rows of those labels.
  int t_lo = 0, t_hi = wk.tn;
  if (use_labels && lab_start != nullptr) {
    if (lane == 0) {
      wrange[0][wave] = wmin;
      wrange[1][wave] = wmax;
    }
    __syncthreads();
    const int bmin = min(min(wrange[0][0], wrange[0][1]), min(wrange[0][2], wrange[0][3]));
    const int bmax = max(max(wrange[1][0], wrange[1][1]), max(wrange[1][2], wrange[1][3]));
    if (bmin > bmax) {
      t_hi = 0;  // no query of this workgroup has a part
    } else {
      t_lo = lab_start[wk.pad * 10 + bmin];
      t_hi = lab_start[wk.pad * 10 + bmax + 1];
    }
  }
  double bd[KNM_NG][KNM_KK], pd[KNM_NG][KNM_PEND];
  int32_t bi[KNM_NG][KNM_KK], pi[KNM_NG][KNM_PEND];
  int pn[KNM_NG];
#pragma unroll
  for (int g = 0; g < KNM_NG; ++g) {
    pn[g] = 0;
#pragma unroll
    for (int j = 0; j < KNM_KK; ++j) {
      bd[g][j] = INFINITY;
      bi[g][j] = 0x7fffffff;
    }
#pragma unroll
    for (int j = 0; j < KNM_PEND; ++j) {
      pd[g][j] = INFINITY;
      pi[g][j] = 0x7fffffff;
    }
  }
  auto rank_pending = [&](int g) {
#pragma unroll
    for (int e = 0; e < KNM_PEND; ++e) {
      double cd = pd[g][e];  // +inf in unused slots: never inserted
      int32_t ci = pi[g][e];
      pd[g][e] = INFINITY;
      if (cd < bd[g][KNM_KK - 1]) {
        bool carry = false;
#pragma unroll
        for (int s2 = 0; s2 < KNM_KK; ++s2) {
          if (carry || cd < bd[g][s2]) {
            carry = true;
            const double td = bd[g][s2];
            const int32_t ti = bi[g][s2];
            bd[g][s2] = cd;
            bi[g][s2] = ci;
            cd = td;
            ci = ti;
          }
        }
      }
    }
    pn[g] = 0;
  };
  // staging registers: thread tid owns row tid of the stage
  float4 sf[4];
  double sn;
  int32_t sl, si;
  auto stage_load = [&](int tbase) {
    const int j = tid;
    const bool ok = tbase + j < t_hi;
    const int src = ok ? (torder ? torder[wk.t0 + tbase + j] : tbase + j) : 0;
    const float4* rp = reinterpret_cast<const float4*>(tf + (wk.t0 + src) * 16);
#pragma unroll
    for (int c = 0; c < 4; ++c) sf[c] = rp[c];
    sn = ok ? tnorm[wk.t0 + src] : INFINITY;  // +inf distance for rows past the segment
    const int tl = (ok && use_labels) ? tlabel[wk.t0 + src] : (ok ? 0 : 8);
    sl = (tl >= 0 && tl < 8) ? tl : 8;         // 8 = no part: matches no query, sorts last
    si = ok ? src : 0x7fffffff;
  };
  auto stage_store = [&](int b) {
    float2* dst = reinterpret_cast<float2*>(&t_lds[b][tid * KNM_PITCH]);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      dst[2 * c] = make_float2(sf[c].x, sf[c].y);
      dst[2 * c + 1] = make_float2(sf[c].z, sf[c].w);
    }
    tn_lds[b][tid] = sn;
    tl_lds[b][tid] = sl;
    ti_lds[b][tid] = si;
  };
  double thr = INFINITY;  // pruning threshold of the lane's query (see the ranking step below)
  if (t_hi > t_lo) {
    stage_load(t_lo);
    stage_store(0);
  }
  __syncthreads();
  int buf = 0;
  for (int tbase = t_lo; tbase < t_hi; tbase += KNM_TT) {
    const int tcount = min(KNM_TT, t_hi - tbase);
    const bool more = tbase + KNM_TT < t_hi;
    if (more) stage_load(tbase + KNM_TT);  // global loads in flight during the tiles below
    // two 16-row tiles per iteration: their MFMA chains are independent, so the second chain issues
    // while the first drains, and the LDS reads of both are in flight together (rows past tcount carry
    // |t|^2 = +inf and never enter a shortlist)
    static_assert(KNM_NG == 1, "the two-tile loop below is written for one query group per wave");
    for (int t = 0; t < (tcount + 15) / 16; t += 2) {
      const float* ap = &t_lds[buf][(16 * t + col) * KNM_PITCH + kq];
      double a0[4], a1[4];
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        a0[s4] = (double)ap[4 * s4];                        // A[target row][k = 4 s + kq]
        a1[s4] = (double)ap[16 * KNM_PITCH + 4 * s4];
      }
      f64x4 acc0, acc1;
      int tl0[4], tl1[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc0[r] = tn_lds[buf][16 * t + kq + 4 * r];
        acc1[r] = tn_lds[buf][16 * t + 16 + kq + 4 * r];
        tl0[r] = tl_lds[buf][16 * t + kq + 4 * r];
        tl1[r] = tl_lds[buf][16 * t + 16 + kq + 4 * r];
      }
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[s4], qb[0][s4], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[s4], qb[0][s4], acc1, 0, 0, 0);
      }
      // acc[r] = |t|^2 - 2 q.t for target row 16 t (+16) + kq + 4 r and the lane's query
#pragma unroll
      for (int u = 0; u < 2; ++u) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          double dist = u ? acc1[r] : acc0[r];
          if (use_labels && (u ? tl1[r] : tl0[r]) != want[0]) dist = INFINITY;
          if (dist < thr) {
#pragma unroll
            for (int e = KNM_PEND - 1; e > 0; --e) {
              pd[0][e] = pd[0][e - 1];
              pi[0][e] = pi[0][e - 1];
            }
            pd[0][0] = dist;
            pi[0][0] = ti_lds[buf][16 * t + 16 * u + kq + 4 * r];
            ++pn[0];
          }
          if (__any(pn[0] == KNM_PEND)) {
            rank_pending(0);
            // The four lanes of a query (kq = 0..3) scan disjoint quarters of the targets.  Whichever of
            // them already holds KNM_KK candidates below tau bounds the query's KNM_KK-th best by tau,
            // so all four may prune with the smallest of their KNM_KK-th values.
            thr = bd[0][KNM_KK - 1];
            thr = fmin(thr, __shfl_xor(thr, 16));
            thr = fmin(thr, __shfl_xor(thr, 32));
          }
        }
      }
    }
    if (more) stage_store(buf ^ 1);
    __syncthreads();
    buf ^= 1;
  }
#pragma unroll
  for (int g = 0; g < KNM_NG; ++g) {
    rank_pending(g);
    const int qloc = wave * 16 * KNM_NG + 16 * g + col;
    if (qvalid[g]) {
      const int64_t base = ((wk.o0 + qloc) * 4 + kq) * KNM_KK;
#pragma unroll
      for (int j = 0; j < KNM_KK; ++j) cand_i[base + j] = bi[g][j];
    }
  }
}

// One thread per query: canonical distances of its 4 * KNM_KK candidates, k best by (distance, row).
__global__ void k_knn_rescore16(const KnnWork* __restrict__ work, const float* __restrict__ qf,
                                const float* __restrict__ tf, const int32_t* __restrict__ cand_i,
                                int k, int32_t* __restrict__ out_idx, double* __restrict__ out_dist,
                                int32_t* __restrict__ qflag, int32_t* __restrict__ tile_flag) {
  const KnnWork wk = work[blockIdx.x];
  const int qloc = threadIdx.x;
  if (qloc >= wk.qn) return;
  const int64_t qrow = wk.q0 + qloc;
  double q[16], qn2 = 0.0;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    q[c] = (double)qf[qrow * 16 + c];
    qn2 = fma(q[c], q[c], qn2);
  }
  // Range of the expansion.  |t|^2 - 2 q.t carries a rounding of ~2^-52 (|q| + |t|)^2: a query far outside the unit
  // range (1e30 in one element: every canonical distance rounds to the same 1e60 and the (distance, row) rule decides,
  // while the expansion still ranks by -2 q.t) or a non-finite one (every value NaN: an empty shortlist) is not
  // shortlisted at all but recomputed by k_knn_feat<16>, like the queries the f16 path cannot verify.  A target row
  // only affects its own value: a NaN / inf row is never shortlisted, a huge finite one ranks last, as it should.
  const bool bad = !(qn2 < KNF_RANGE);
  qflag[wk.o0 + qloc] = bad ? 1 : 0;
  if (bad) atomicOr(&tile_flag[blockIdx.x], 1);
  double bd[KNN_MAXK];
  int32_t bi[KNN_MAXK];
#pragma unroll
  for (int j = 0; j < KNN_MAXK; ++j) {
    bd[j] = INFINITY;
    bi[j] = 0x7fffffff;
  }
  const int32_t* ci = cand_i + (wk.o0 + qloc) * 4 * KNM_KK;
  for (int c = 0; c < 4 * KNM_KK; ++c) {
    const int32_t row = ci[c];
    if (row == 0x7fffffff) continue;
    const float* tp = tf + (wk.t0 + row) * 16;
    double d = 0.0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const double diff = q[e] - (double)tp[e];
      d = fma(diff, diff, d);
    }
    // ordered insertion by (d, row)
    double cd = d;
    int32_t cr = row;
    bool carry = false;
#pragma unroll
    for (int s2 = 0; s2 < KNN_MAXK; ++s2) {
      if (carry || cd < bd[s2] || (cd == bd[s2] && cr < bi[s2])) {
        carry = true;
        const double td = bd[s2];
        const int32_t ti = bi[s2];
        bd[s2] = cd;
        bi[s2] = cr;
        cd = td;
        cr = ti;
      }
    }
  }
  const int64_t orow = wk.o0 + qloc;
  for (int j = 0; j < k; ++j) {
    double dj = INFINITY;
    int32_t ij = 0x7fffffff;
#pragma unroll
    for (int s2 = 0; s2 < KNN_MAXK; ++s2)
      if (s2 == j) {
        dj = bd[s2];
        ij = bi[s2];
      }
    const bool have = ij != 0x7fffffff;
    out_idx[orow * k + j] = have ? ij : -1;
    if (out_dist) out_dist[orow * k + j] = have ? sqrt(dj) : INFINITY;
  }
}

// ------------------------------------------------------------------------------------------
// feature k-NN shortlist on the f16 matrix cores (16-d features, k <= 6): the default path.
// On gfx950 the f64 MFMA runs on the vector unit's double-precision ALUs (78.6 TF either way; measured:
// the f64-MFMA kernel above cannot overlap its MFMAs with its own VALU work), so it stays ~3x above its
// bound.  Here |t|^2 - 2 q.t is evaluated like the RANSAC prefilter: every feature is split into f16
// hi + lo, hi*hi + lo*hi + hi*lo (48 products) is three v_mfma_f32_32x32x16_f16 per 32 x 32 tile (true
// matrix cores, ~20x the f64 rate, co-issuing with the VALU), the accumulator is preloaded with |t|^2.
//   rows = targets (LDS, staged by LDS-DMA from a 112-B-pitch f16 image in visiting order),
//   cols = queries (registers): a lane owns one query and 16 of the tile's 32 target rows.
// The result is only a SHORTLIST (2 x KNF_KK candidates per query by the approximate value).
// k_knn_rescore_f16 re-evaluates them with the canonical f64 chain, ranks by (distance, row) and
// VERIFIES the shortlist: every target that was not kept has an approximate value >= tau (the final
// pruning threshold), hence an exact one >= tau - eps; if the exact k-th distance is not below that,
// the query is flagged and recomputed by the exhaustive kernel (k_knn_feat<16>, flagged tiles only).
// The answer therefore equals the exhaustive kernel's for every query.
// ------------------------------------------------------------------------------------------
// (KNF_PITCH, KNF_ROWS, the operand rows, the stage and tile helpers and the error budget: nn_common.h, shared with hardneg.hip)
constexpr int KNF_NG = 2;       // 32-query groups per wave
constexpr int KNF_QT = 4 * 32 * KNF_NG;  // queries per workgroup
static_assert(KNF_QT == 256, "tiles of the f16 path and of the exhaustive fallback must coincide");
constexpr int KNF_KK = 8;       // shortlist per lane (two lanes per query); 6 was measured: 23 of 189 517 queries fail the
                                // verification and their exhaustive recomputation costs more than the shorter lists save
constexpr int KNF_PEND = 4;

// target image: row j of the image = target (t0 + torder[t0 + j]) (or t0 + j): [th(16) | tl(16) | th(16) | 0(8)],
// tn32 = |t|^2 (f64 chain, rounded up to f32 is not needed: the verification budget covers its rounding),
// ti32 = row local to the segment.  seg_t2max[seg] = max |t|^2 (error budget of the verification).
__global__ void k_knf_pack_targets(const float* __restrict__ tf, const int64_t* __restrict__ toff, int n_seg,
                                   const int32_t* __restrict__ torder, _Float16* __restrict__ img,
                                   float* __restrict__ tn32, int32_t* __restrict__ ti32,
                                   unsigned* __restrict__ seg_t2max_bits) {
  const int sg = blockIdx.y;
  const int64_t b = toff[sg], e = toff[sg + 1];
  float mx = 0.f;
  for (int64_t j = b + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < e; j += (int64_t)gridDim.x * blockDim.x) {
    const int32_t loc = torder ? torder[j] : (int32_t)(j - b);
    const double n2 = knf_pack_target_row(tf + (b + loc) * 16, img + j * KNF_PITCH);
    tn32[j] = (float)n2;
    ti32[j] = loc;
    mx = fmaxf(mx, (float)n2 * 1.0000002f);
  }
  knf_seg_max(mx, &seg_t2max_bits[sg]);
}

// query operand rows: [-2 qh(16) | -2 qh(16) | -2 ql(16)] (scaling by 2 is exact in f16 below the range limit)
__global__ void k_knf_pack_queries(const float* __restrict__ qf, int64_t n, _Float16* __restrict__ qrows,
                                   float* __restrict__ qn32) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double n2 = knf_pack_query_row(qf + i * 16, qrows + i * 48);
  qn32[i] = (float)n2 * 1.0000002f;   // |q|^2, rounded up: error budget of the threshold pass
}

// PASS = 1 (round 5): the THRESHOLD pass.  The shortlist kernel is bound by its hits, not by the matrix cores (MFMA busy
// 0.07): a lane starts with thr = +inf, its running 8th best falls like a record process (~55 hits per lane, and with 64
// lanes a hit in SOME lane on 70 % of the value steps), and every hit step pays the pending list and its ranking.  This pass
// bounds the query's k-th distance BEFORE the shortlist pass from tile minima alone -- no per-value work: one MFMA (hi.hi,
// 16 of the 48 products) per 32 x 32 tile, eight v_min3 for the tile's minimum of the lane's 16 rows, six v_med3 to keep the
// lane's six smallest tile minima.  The k-th smallest b_k is attained by k DIFFERENT rows, so the exact k-th distance is
// <= b_k + eps1 and every true neighbour has a full approximate value <= b_k + eps1 + eps3 =: thr0 -- the shortlist pass then
// starts from thr0 instead of +inf and sees ~8 hits per lane.  eps1 = 2^-9 (|q|^2 + |t|^2max) covers the hi.hi-only value
// (2 x 2^-11 relative on either side of q.t, times the factor 2, charged twice), eps3 = 2^-15 (...) the three-MFMA value as in
// k_knn_rescore_f16.  Nothing here decides a result: the shortlist is verified against its final threshold as before and a
// query whose list is short or unverifiable is recomputed exhaustively.
template <int PASS>
__global__ __launch_bounds__(256) void k_knn_f16(const KnnWork* __restrict__ work,
                                                 const _Float16* __restrict__ qrows,
                                                 const _Float16* __restrict__ img,
                                                 const float* __restrict__ tn32,
                                                 const int32_t* __restrict__ ti32,
                                                 const int32_t* __restrict__ qlabel,
                                                 const int32_t* __restrict__ perm,
                                                 const int32_t* __restrict__ lab_start,
                                                 int32_t* __restrict__ cand_i, float* __restrict__ cand_tau,
                                                 // PASS 1 writes thr0, PASS 0 starts from it (nullptr: from +inf)
                                                 float* __restrict__ thr0, const float* __restrict__ qn32,
                                                 const unsigned* __restrict__ seg_t2max_bits, int kq) {
  constexpr int STAGE_BYTES = KNF_STAGE_BYTES;
  __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE_BYTES];
  __shared__ __attribute__((aligned(16))) float tn_s[2][KNF_ROWS];
  __shared__ int32_t wrange[2][4];
  const KnnWork wk = work[blockIdx.x];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int col = lane & 31;
  const bool use_labels = qlabel != nullptr;
  f16x8 bop[KNF_NG][3];
  int want[KNF_NG];
  bool qvalid[KNF_NG];
  int wmin = 0x7fffffff, wmax = -2;
#pragma unroll
  for (int g = 0; g < KNF_NG; ++g) {
    const int qloc = wave * 32 * KNF_NG + 32 * g + col;
    qvalid[g] = qloc < wk.qn;
    const int64_t qrow = wk.q0 + (qvalid[g] ? qloc : 0);
    const _Float16* row = qrows + qrow * 48 + 8 * half;
#pragma unroll
    for (int m = 0; m < 3; ++m) bop[g][m] = *reinterpret_cast<const f16x8*>(row + 16 * m);
    want[g] = -1;
    if (use_labels) {
      const int ql = qlabel[qrow];
      want[g] = (qvalid[g] && ql >= 0 && ql < 8) ? perm[wk.prob * 8 + ql] : -2;
      if (want[g] >= 0) wmin = min(wmin, want[g]);
      wmax = max(wmax, want[g]);
    }
  }
  int lab_lo = -1, lab_hi = -1;  // label passes (one pass, label -1, without labels)
  if (use_labels) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      wmin = min(wmin, __shfl_xor(wmin, off));
      wmax = max(wmax, __shfl_xor(wmax, off));
    }
    if (lane == 0) {
      wrange[0][wave] = wmin;
      wrange[1][wave] = wmax;
    }
    __syncthreads();
    lab_lo = min(min(wrange[0][0], wrange[0][1]), min(wrange[0][2], wrange[0][3]));
    lab_hi = max(max(wrange[1][0], wrange[1][1]), max(wrange[1][2], wrange[1][3]));
    if (lab_hi > 7) lab_hi = 7;
    if (lab_lo > lab_hi) lab_hi = lab_lo - 1;  // nothing to scan
  }
  // ranked shortlist + pending list per lane and group (see k_knn_mfma16 for the scheme)
  float bd[KNF_NG][KNF_KK], pd[KNF_NG][KNF_PEND], thr[KNF_NG];
  int32_t bi[KNF_NG][KNF_KK], pi[KNF_NG][KNF_PEND];
  int pn[KNF_NG];
  float tb[KNF_NG][6];   // PASS 1: the lane's six smallest tile minima, ascending
#pragma unroll
  for (int g = 0; g < KNF_NG; ++g) {
    pn[g] = 0;
    thr[g] = INFINITY;
    if (PASS == 0 && thr0) {
      const int qloc = wave * 32 * KNF_NG + 32 * g + col;
      thr[g] = thr0[wk.o0 + (qvalid[g] ? qloc : 0)];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) tb[g][j] = INFINITY;
#pragma unroll
    for (int j = 0; j < KNF_KK; ++j) {
      bd[g][j] = INFINITY;
      bi[g][j] = 0x7fffffff;
    }
#pragma unroll
    for (int j = 0; j < KNF_PEND; ++j) {
      pd[g][j] = INFINITY;
      pi[g][j] = 0x7fffffff;
    }
  }
  auto rank_pending = [&](int g) {
#pragma unroll
    for (int e = 0; e < KNF_PEND; ++e) {
      float cd = pd[g][e];
      int32_t ci = pi[g][e];
      pd[g][e] = INFINITY;
      if (cd < bd[g][KNF_KK - 1]) knf_insert(bd[g], bi[g], cd, ci);
    }
    pn[g] = 0;
    thr[g] = fminf(thr[g], knf_pair_min(bd[g][KNF_KK - 1]));   // (never above the threshold pass's bound while the lists are still filling)
  };
  const char* gimg = reinterpret_cast<const char*>(img + (int64_t)wk.t0 * KNF_PITCH) + lane * 16;
  const unsigned lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(lds));
  for (int lab = lab_lo; lab <= lab_hi; ++lab) {
    int t_lo = 0, t_hi = wk.tn;
    if (use_labels) {
      if (lab_start == nullptr) break;
      t_lo = lab_start[wk.pad * 10 + lab];
      t_hi = lab_start[wk.pad * 10 + lab + 1];
    }
    if (t_hi <= t_lo) continue;
    float thr_eff[KNF_NG];
#pragma unroll
    for (int g = 0; g < KNF_NG; ++g) thr_eff[g] = (!use_labels || want[g] == lab) ? thr[g] : -INFINITY;
    // (LDS-DMA as inline asm + |t|^2 / row ids loaded before it and stored after the stage's compute: see k_topk_f16)
    auto issue_dma = [&](int b, int base) { knf_issue_dma(gimg, lds_base, wave, b, base); };
    auto load_rows = [&](int base, float& tn) {   // unconditional (clamped) loads
      int r = base + (tid % KNF_ROWS);
      r = r > t_hi - 1 ? t_hi - 1 : r;
      r = r < t_lo ? t_lo : r;
      tn = tn32[wk.t0 + r];
    };
    auto store_rows = [&](int b, int base, float tn) {
      if (tid < KNF_ROWS) tn_s[b][tid] = base + tid < t_hi ? tn : INFINITY;  // rows past the label's range can never be hit
    };
    __syncthreads();  // the previous label pass may still read the buffers
    {
      float tn0;
      load_rows(t_lo, tn0);
      issue_dma(0, t_lo);
      store_rows(0, t_lo, tn0);
    }
    int buf = 0;
    for (int base = t_lo; base < t_hi; base += KNF_ROWS) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const bool more = base + KNF_ROWS < t_hi;
      float tn_next;
      load_rows(base + KNF_ROWS, tn_next);
      if (more) issue_dma(buf ^ 1, base + KNF_ROWS);
#pragma unroll 1
      for (int t = 0; t < KNF_ROWS / 32; ++t) {
        if (base + 32 * t >= t_hi) break;  // whole tile past the range (block-uniform)
        f16x8 a[3];
        f32x16 c16;
        knf_load_tile(lds + buf * STAGE_BYTES, tn_s[buf], t, col, half, a, c16);
#pragma unroll
        for (int g = 0; g < KNF_NG; ++g) {
          f32x16 d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], bop[g][0], c16, 0, 0, 0);
          if (PASS == 1) {
            float m = fminf(fminf(d[0], d[1]), d[2]);
            m = fminf(fminf(m, d[3]), d[4]);
            m = fminf(fminf(m, d[5]), d[6]);
            m = fminf(fminf(m, d[7]), d[8]);
            m = fminf(fminf(m, d[9]), d[10]);
            m = fminf(fminf(m, d[11]), d[12]);
            m = fminf(fminf(m, d[13]), d[14]);
            m = fminf(m, d[15]);
            if (use_labels && want[g] != lab) m = INFINITY;
            // sorted insertion without a branch: new j-th = median of (old j-1-th, old j-th, m)
            const float o0 = tb[g][0], o1 = tb[g][1], o2 = tb[g][2], o3 = tb[g][3], o4 = tb[g][4], o5 = tb[g][5];
            tb[g][0] = fminf(o0, m);
            tb[g][1] = __builtin_amdgcn_fmed3f(o0, o1, m);
            tb[g][2] = __builtin_amdgcn_fmed3f(o1, o2, m);
            tb[g][3] = __builtin_amdgcn_fmed3f(o2, o3, m);
            tb[g][4] = __builtin_amdgcn_fmed3f(o3, o4, m);
            tb[g][5] = __builtin_amdgcn_fmed3f(o4, o5, m);
            continue;
          }
          d = knf_mfma_lo(a, bop[g], d);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            // one compare + one scalar branch per value while no lane of the wave has a hit (three of four values
            // once a few hundred targets have been seen); the pending-list push only runs behind it
#ifdef KNF_NOHIT
            const bool hit = d[r] < thr_eff[g] - 1.0e30f;
#else
            const bool hit = d[r] < thr_eff[g];
#endif
            if (__any(hit)) {
              if (hit) {
#pragma unroll
                for (int e = KNF_PEND - 1; e > 0; --e) {
                  pd[g][e] = pd[g][e - 1];
                  pi[g][e] = pi[g][e - 1];
                }
                pd[g][0] = d[r];
                pi[g][0] = base + knf_result_row(t, half, r);   // position in the image; its row id is looked up at the end
                ++pn[g];
              }
              if (__any(pn[g] == KNF_PEND)) {
                rank_pending(g);
                thr_eff[g] = (!use_labels || want[g] == lab) ? thr[g] : -INFINITY;
              }
            }
          }
        }
      }
      if (more) store_rows(buf ^ 1, base + KNF_ROWS, tn_next);
      buf ^= 1;
    }
  }
  if (PASS == 1) {
#pragma unroll
    for (int g = 0; g < KNF_NG; ++g) {
      float bk = INFINITY;
#pragma unroll
      for (int j = 0; j < 6; ++j)
        if (j == kq - 1) bk = tb[g][j];
      bk = fminf(bk, __shfl_xor(bk, 32));     // either lane's k-th smallest tile minimum bounds the query's k-th value
      const int qloc = wave * 32 * KNF_NG + 32 * g + col;
      if (qvalid[g] && half == 0) {
        const float budget = qn32[wk.q0 + qloc] + __uint_as_float(seg_t2max_bits[wk.pad]);
        // (+ eps1 + eps3, rounded up, and strictly above every value it has to admit)
        thr0[wk.o0 + qloc] = bk + budget * (0x1.0p-9f + 0x1.0p-14f) + fabsf(bk) * 0x1.0p-20f;
      }
    }
    return;
  }
#pragma unroll
  for (int g = 0; g < KNF_NG; ++g) {
    rank_pending(g);
    const int qloc = wave * 32 * KNF_NG + 32 * g + col;
    if (qvalid[g]) {
      const int64_t base = ((wk.o0 + qloc) * 2 + half) * KNF_KK;
      // shortlist entries are positions in the target image (no LDS read on the hit path): row ids only now
#pragma unroll
      for (int j = 0; j < KNF_KK; ++j) cand_i[base + j] = bi[g][j] != 0x7fffffff ? ti32[wk.t0 + bi[g][j]] : 0x7fffffff;
      if (half == 0) cand_tau[wk.o0 + qloc] = thr[g];
    }
  }
}

// One thread per query: canonical distances of its 2 * KNF_KK candidates, k best by (distance, row), and
// the verification of the shortlist (see the header of this section).  flag[tile] != 0 -> k_knn_feat
// recomputes that tile's flagged queries exhaustively.
__global__ void k_knn_rescore_f16(const KnnWork* __restrict__ work, const float* __restrict__ qf,
                                  const float* __restrict__ tf, const int32_t* __restrict__ cand_i,
                                  const float* __restrict__ cand_tau,
                                  const unsigned* __restrict__ seg_t2max_bits, int k,
                                  int32_t* __restrict__ out_idx, double* __restrict__ out_dist,
                                  int32_t* __restrict__ qflag, int32_t* __restrict__ tile_flag) {
  const KnnWork wk = work[blockIdx.x];
  const int qloc = threadIdx.x;
  if (qloc >= wk.qn) return;
  const int64_t qrow = wk.q0 + qloc;
  double q[16], qn2 = 0.0;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    q[c] = (double)qf[qrow * 16 + c];
    qn2 = fma(q[c], q[c], qn2);
  }
  double bd[KNN_MAXK];
  int32_t bi[KNN_MAXK];
#pragma unroll
  for (int j = 0; j < KNN_MAXK; ++j) {
    bd[j] = INFINITY;
    bi[j] = 0x7fffffff;
  }
  const int32_t* ci = cand_i + (wk.o0 + qloc) * 2 * KNF_KK;
  int n_cand = 0;
  for (int c = 0; c < 2 * KNF_KK; ++c) {
    const int32_t row = ci[c];
    if (row == 0x7fffffff) continue;
    ++n_cand;
    double cd = knf_chain16(q, tf + (wk.t0 + row) * 16);
    int32_t cr = row;
    bool carry = false;
#pragma unroll
    for (int s2 = 0; s2 < KNN_MAXK; ++s2) {
      if (carry || cd < bd[s2] || (cd == bd[s2] && cr < bi[s2])) {
        carry = true;
        const double td = bd[s2];
        const int32_t ti = bi[s2];
        bd[s2] = cd;
        bi[s2] = cr;
        cd = td;
        cr = ti;
      }
    }
  }
  const int64_t orow = wk.o0 + qloc;
  double dk = INFINITY;  // exact k-th distance
  for (int j = 0; j < k; ++j) {
    double dj = INFINITY;
    int32_t ij = 0x7fffffff;
#pragma unroll
    for (int s2 = 0; s2 < KNN_MAXK; ++s2)
      if (s2 == j) {
        dj = bd[s2];
        ij = bi[s2];
      }
    const bool have = ij != 0x7fffffff;
    out_idx[orow * k + j] = have ? ij : -1;
    if (out_dist) out_dist[orow * k + j] = have ? sqrt(dj) : INFINITY;
    dk = dj;
  }
  // Verification.  Targets that were dropped have approximate value >= tau, i.e. exact
  // |t|^2 - 2 q.t >= tau - eps with eps covering: 48 f32 accumulation steps and the dropped lo*lo
  // products relative to sum |terms| <= |q|^2 + |t|^2, the hi+lo split residuals, the f32 rounding of
  // |t|^2 -- together < 2^-17 (|q|^2 + |t|^2_max); charged 2^-15.  If the shortlists were never filled
  // (tau = +inf) every target of the query's part is a candidate and nothing was dropped.
  const float tau = cand_tau[orow];
  const double t2max = (double)__uint_as_float(seg_t2max_bits[wk.pad]);
  const double eps = KNF_EPS_REL * (qn2 + t2max);
  bool ok = true;
  if (tau < INFINITY) {
    // need: exact k-th (as |t|^2 - 2 q.t = d - |q|^2) strictly below every dropped target's exact value;
    // equality would need the (distance, row) tie rule, which the shortlist does not know
    ok = n_cand >= k && (dk - qn2) < (double)tau - eps;
  }
  if (!(qn2 < KNF_RANGE) || !(t2max < KNF_RANGE)) ok = false;  // outside the f16 range: not trusted at all
  qflag[orow] = ok ? 0 : 1;
  if (!ok) atomicOr(&tile_flag[blockIdx.x], 1);
}

}  // namespace cs

using namespace cs;

// {queries answered by the f16 shortlist path, of those recomputed exhaustively}; counted only while
// CS_KNN_STATS=1 (the count costs a synchronisation)
static std::atomic<unsigned long long> g_knn_stats[2];

__global__ void k_count_flags(const int32_t* __restrict__ flag, int64_t n, unsigned long long* __restrict__ out) {
  int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  unsigned long long v = (i < n && flag[i]) ? 1ULL : 0ULL;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}

int cs::count_flagged(const int32_t* d_flag, int64_t n, unsigned long long* host_out, hipStream_t s,
                      const char* who) {
  PoolBuf<unsigned long long> cnt(1);
  CS_REQUIRE(cnt.p, CS_ERR_HIP, "%s: scratch allocation failed", who);
  CS_HIP_CHECK(hipMemsetAsync(cnt.p, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_count_flags, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, s, d_flag, n, cnt.p);
  CS_HIP_CHECK(hipMemcpyAsync(host_out, cnt.p, sizeof(*host_out), hipMemcpyDeviceToHost, s));
  CS_HIP_CHECK(hipStreamSynchronize(s));
  return CS_OK;
}

// The environment switches of cs_knn_feat.
struct KnnOptions {
  enum Path { F16, F64, EXHAUSTIVE };
  Path path;      // CS_KNN_MFMA: unset f16 matrix-core shortlist, "64" f64 matrix-pipe shortlist, "0" exhaustive VALU kernel
  bool two_pass;  // CS_KNN_TWOPASS=0: the f16 shortlist pass alone, from +inf (no threshold pass)
  bool stats;     // CS_KNN_STATS=1: count the queries the f16 path recomputed exhaustively (synchronises)
};
static KnnOptions read_options() {
  const char* mfma = getenv("CS_KNN_MFMA");
  KnnOptions o;
  o.path = KnnOptions::F16;
  if (mfma && mfma[0] == '0') o.path = KnnOptions::EXHAUSTIVE;
  if (mfma && mfma[0] == '6') o.path = KnnOptions::F64;
  o.two_pass = !env_first_is("CS_KNN_TWOPASS", '0');
  o.stats = env_first_is("CS_KNN_STATS", '1');
  return o;
}

// What cs_knn_feat has checked and built before it hands the call to one of the three paths.
struct KnnCall {
  const float *d_qf, *d_tf;
  const int64_t *h_qoff, *h_toff;
  int nqseg, ntseg;      // segments the problems refer to: rows [0, h_qoff[nqseg]) and [0, h_toff[ntseg])
  int dim, k;
  const int32_t *d_qlabel, *d_tlabel, *d_perm;
  int32_t* d_idx;
  double* d_dist;
  const KnnWork* d_work;
  unsigned n_work;
  int64_t out_row;       // output rows (queries of all problems)
  double flop;
  hipStream_t s;
};

// Label order of every target segment (stable: equal labels keep their row order): torder[position] = row local to
// the segment, lab_start[seg * 10 + l] = first position whose label key is >= l.
static int label_order(const int32_t* d_tlabel, const int64_t* d_toff, int ntseg, int64_t nt_rows, hipStream_t s,
                       PoolBuf<int32_t>& torder, PoolBuf<int32_t>& lab_start) {
  PoolBuf<int32_t> rows_in;
  PoolBuf<uint32_t> keys, keys_sorted;
  PoolBuf<char> tmp;
  CS_REQUIRE(torder.alloc((size_t)nt_rows) && keys.alloc((size_t)nt_rows) && keys_sorted.alloc((size_t)nt_rows) &&
                 rows_in.alloc((size_t)nt_rows) && lab_start.alloc((size_t)ntseg * 10),
             CS_ERR_HIP, "cs_knn_feat: scratch allocation failed");
  hipLaunchKernelGGL(k_seg_keys, dim3(16, (unsigned)ntseg), dim3(256), 0, s, d_toff, ntseg, d_tlabel, keys.p,
                     rows_in.p);
  int end_bit = 4;
  while ((1LL << end_bit) < (int64_t)ntseg * 16) ++end_bit;
  size_t tmp_bytes = 0;
  CS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys.p, keys_sorted.p, rows_in.p, torder.p,
                                                  (int)nt_rows, 0, end_bit, s));
  CS_REQUIRE(tmp.alloc(tmp_bytes ? tmp_bytes : 1), CS_ERR_HIP, "cs_knn_feat: scratch allocation failed");
  CS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys.p, keys_sorted.p, rows_in.p, torder.p,
                                                  (int)nt_rows, 0, end_bit, s));
  hipLaunchKernelGGL(k_label_starts, dim3((unsigned)ceil_div((int64_t)ntseg * 10, 256)), dim3(256), 0, s, d_toff,
                     ntseg, keys_sorted.p, lab_start.p);
  return CS_OK;
}

// 16-d, k <= 6, the default: f16 matrix-core shortlist (k_knn_f16), canonical rescore and verification
// (k_knn_rescore_f16), exhaustive recomputation of the queries that fail it (k_knn_feat<16>, flagged tiles only)
static int knn_f16(const KnnCall& c, const KnnOptions& opt) {
  hipStream_t s = c.s;
  const int64_t nq_rows = c.h_qoff[c.nqseg], nt_rows = c.h_toff[c.ntseg], out_row = c.out_row;
  const int ntseg = c.ntseg;
  CS_REQUIRE(nt_rows < (1LL << 31) && ntseg < (1 << 27), CS_ERR_UNSUPPORTED,
             "cs_knn_feat: too many target rows / segments");
  PoolBuf<_Float16> qrows((size_t)(nq_rows ? nq_rows : 1) * 48);
  PoolBuf<_Float16> img((size_t)(nt_rows + KNF_ROWS) * KNF_PITCH);  // + one stage of slack for the last copy
  PoolBuf<float> tn32((size_t)(nt_rows ? nt_rows : 1)), tau((size_t)(out_row ? out_row : 1));
  PoolBuf<int32_t> ti32((size_t)(nt_rows ? nt_rows : 1)), cand((size_t)(out_row ? out_row : 1) * 2 * KNF_KK);
  PoolBuf<int32_t> qflag((size_t)(out_row ? out_row : 1)), tile_flag(c.n_work);
  PoolBuf<unsigned> t2max((size_t)ntseg);
  // threshold pass (k_knn_f16<1>): per query an upper bound of its k-th distance before the shortlist pass starts
  const bool two_pass = c.k <= 6 && opt.two_pass;
  PoolBuf<float> thr0((size_t)(out_row ? out_row : 1)), qn32((size_t)(nq_rows ? nq_rows : 1));
  PoolBuf<int32_t> torder, lab_start;
  PoolBuf<int64_t> dtoff;
  CS_REQUIRE(qrows.p && img.p && tn32.p && tau.p && ti32.p && cand.p && qflag.p && tile_flag.p && t2max.p && thr0.p &&
                 qn32.p,
             CS_ERR_HIP, "cs_knn_feat: scratch allocation failed");
  std::vector<int64_t> toff(c.h_toff, c.h_toff + ntseg + 1);
  int rc = upload(dtoff, toff, s);
  if (rc) return rc;
  const bool labelled = c.d_tlabel && nt_rows;
  if (labelled) {
    rc = label_order(c.d_tlabel, dtoff.p, ntseg, nt_rows, s, torder, lab_start);
    if (rc) return rc;
  }
  CS_HIP_CHECK(hipMemsetAsync(t2max.p, 0, sizeof(unsigned) * ntseg, s));
  CS_HIP_CHECK(hipMemsetAsync(tile_flag.p, 0, sizeof(int32_t) * c.n_work, s));
  if (nt_rows)
    hipLaunchKernelGGL(k_knf_pack_targets, dim3(16, (unsigned)ntseg), dim3(256), 0, s, c.d_tf, dtoff.p, ntseg,
                       labelled ? torder.p : (const int32_t*)nullptr, img.p, tn32.p, ti32.p, t2max.p);
  if (nq_rows)
    hipLaunchKernelGGL(k_knf_pack_queries, dim3((unsigned)ceil_div(nq_rows, 256)), dim3(256), 0, s, c.d_qf, nq_rows,
                       qrows.p, qn32.p);
  {
    ProfScope prof("knn", s, c.flop);
    const dim3 grid(c.n_work);
    const int32_t* labs = labelled ? lab_start.p : (const int32_t*)nullptr;
    if (two_pass)
      hipLaunchKernelGGL(k_knn_f16<1>, grid, dim3(256), 0, s, c.d_work, qrows.p, img.p, tn32.p, ti32.p, c.d_qlabel,
                         c.d_perm, labs, cand.p, tau.p, thr0.p, qn32.p, t2max.p, c.k);
    hipLaunchKernelGGL(k_knn_f16<0>, grid, dim3(256), 0, s, c.d_work, qrows.p, img.p, tn32.p, ti32.p, c.d_qlabel,
                       c.d_perm, labs, cand.p, tau.p, two_pass ? thr0.p : (float*)nullptr, qn32.p, t2max.p, c.k);
    hipLaunchKernelGGL(k_knn_rescore_f16, grid, dim3(256), 0, s, c.d_work, c.d_qf, c.d_tf, cand.p, tau.p, t2max.p,
                       c.k, c.d_idx, c.d_dist, qflag.p, tile_flag.p);
    // exhaustive recomputation of the queries whose shortlist could not be verified (normally none)
    hipLaunchKernelGGL((k_knn_feat<16>), grid, dim3(256), 0, s, c.d_work, c.d_qf, c.d_tf, c.k, c.d_qlabel,
                       c.d_tlabel, c.d_perm, c.d_idx, c.d_dist, tile_flag.p, qflag.p);
    CS_LAUNCH_CHECK();
  }
  if (opt.stats && out_row > 0) {
    unsigned long long h = 0;
    rc = count_flagged(qflag.p, out_row, &h, s, "cs_knn_feat");
    if (rc) return rc;
    g_knn_stats[0] += (unsigned long long)out_row;
    g_knn_stats[1] += h;
  }
  return CS_OK;
}

// CS_KNN_MFMA=64: f64 matrix-pipe shortlist (k_knn_mfma16) and canonical rescore (k_knn_rescore16)
static int knn_f64(const KnnCall& c) {
  hipStream_t s = c.s;
  const int64_t nq_rows = c.h_qoff[c.nqseg], nt_rows = c.h_toff[c.ntseg], out_row = c.out_row;
  const int ntseg = c.ntseg;
  CS_REQUIRE(nt_rows < (1LL << 31) && ntseg < (1 << 27), CS_ERR_UNSUPPORTED,
             "cs_knn_feat: too many target rows / segments");
  PoolBuf<double> qnorm((size_t)(nq_rows ? nq_rows : 1)), tnorm((size_t)(nt_rows ? nt_rows : 1));
  PoolBuf<int32_t> cand((size_t)(out_row ? out_row : 1) * 4 * KNM_KK);
  PoolBuf<int32_t> qflag((size_t)(out_row ? out_row : 1)), tile_flag(c.n_work);
  PoolBuf<int32_t> torder, lab_start;
  PoolBuf<int64_t> dtoff;
  CS_REQUIRE(qnorm.p && tnorm.p && cand.p && qflag.p && tile_flag.p, CS_ERR_HIP,
             "cs_knn_feat: scratch allocation failed");
  CS_HIP_CHECK(hipMemsetAsync(tile_flag.p, 0, sizeof(int32_t) * c.n_work, s));
  if (nq_rows) row_norms(c.d_qf, nq_rows, 16, qnorm.p, s);
  if (nt_rows) row_norms(c.d_tf, nt_rows, 16, tnorm.p, s);
  if (c.d_tlabel && nt_rows) {
    std::vector<int64_t> toff(c.h_toff, c.h_toff + ntseg + 1);
    int rc = upload(dtoff, toff, s);
    if (!rc) rc = label_order(c.d_tlabel, dtoff.p, ntseg, nt_rows, s, torder, lab_start);
    if (rc) return rc;
  }
  ProfScope prof("knn", s, c.flop);
  hipLaunchKernelGGL(k_knn_mfma16, dim3(c.n_work), dim3(256), 0, s, c.d_work, c.d_qf, c.d_tf, qnorm.p, tnorm.p,
                     c.d_qlabel, c.d_tlabel, c.d_perm, c.d_tlabel ? torder.p : nullptr,
                     c.d_tlabel ? lab_start.p : nullptr, cand.p);
  hipLaunchKernelGGL(k_knn_rescore16, dim3(c.n_work), dim3(KNM_QT), 0, s, c.d_work, c.d_qf, c.d_tf, cand.p, c.k,
                     c.d_idx, c.d_dist, qflag.p, tile_flag.p);
  // exhaustive recomputation of the queries outside the expansion's range (normally none)
  hipLaunchKernelGGL((k_knn_feat<16>), dim3(c.n_work), dim3(256), 0, s, c.d_work, c.d_qf, c.d_tf, c.k, c.d_qlabel,
                     c.d_tlabel, c.d_perm, c.d_idx, c.d_dist, tile_flag.p, qflag.p);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

// CS_KNN_MFMA=0, and every shape the shortlists do not take (3-d, 32-d, k > 6): the exhaustive VALU kernel
static int knn_exhaustive(const KnnCall& c) {
  ProfScope prof("knn", c.s, c.flop);
  const dim3 grid(c.n_work);
  const int32_t* none = nullptr;
  if (c.dim == 16)
    hipLaunchKernelGGL((k_knn_feat<16>), grid, dim3(256), 0, c.s, c.d_work, c.d_qf, c.d_tf, c.k, c.d_qlabel,
                       c.d_tlabel, c.d_perm, c.d_idx, c.d_dist, none, none);
  else if (c.dim == 32)
    hipLaunchKernelGGL((k_knn_feat<32>), grid, dim3(256), 0, c.s, c.d_work, c.d_qf, c.d_tf, c.k, c.d_qlabel,
                       c.d_tlabel, c.d_perm, c.d_idx, c.d_dist, none, none);
  else
    hipLaunchKernelGGL((k_knn_feat<3>), grid, dim3(256), 0, c.s, c.d_work, c.d_qf, c.d_tf, c.k, c.d_qlabel,
                       c.d_tlabel, c.d_perm, c.d_idx, c.d_dist, none, none);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

extern "C" {

void cs_knn_shortlist_stats(uint64_t out[2], int reset) { read_stats(g_knn_stats, out, reset); }

// Scratch of every path goes back to this thread's stream-ordered cache when the call returns; outputs are valid in
// stream order.
int cs_knn_feat(const float* d_qf, const int64_t* h_qoff, const float* d_tf,
                const int64_t* h_toff, const int32_t* h_qseg, const int32_t* h_tseg, int n_prob,
                int dim, int k, const int32_t* d_qlabel, const int32_t* d_tlabel,
                const int32_t* d_perm, int32_t* d_idx, double* d_dist, void* stream) {
  CS_REQUIRE(d_qf && d_tf && h_qoff && h_toff && h_qseg && h_tseg && d_idx, CS_ERR_INVALID,
             "cs_knn_feat: NULL argument");
  CS_REQUIRE(k >= 1 && k <= KNN_MAXK, CS_ERR_UNSUPPORTED, "cs_knn_feat: k = %d not in [1, %d]", k,
             KNN_MAXK);
  CS_REQUIRE(dim == 16 || dim == 32 || dim == 3, CS_ERR_UNSUPPORTED,
             "cs_knn_feat: feature dimension %d not supported (3, 16, 32)", dim);
  CS_REQUIRE((d_qlabel == nullptr) == (d_tlabel == nullptr) &&
                 (d_qlabel == nullptr) == (d_perm == nullptr),
             CS_ERR_INVALID, "cs_knn_feat: labels and perm must be given together");
  if (n_prob <= 0) return CS_OK;
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const KnnOptions opt = read_options();
  // the shortlist paths take 16-d features with k <= 6; everything else is the exhaustive kernel's
  const KnnOptions::Path path = (dim == 16 && k <= KNM_KK - 2) ? opt.path : KnnOptions::EXHAUSTIVE;
  const int qtile = path == KnnOptions::F64 ? KNM_QT : 256;
  std::vector<KnnWork> work;
  int64_t out_row = 0;
  int nqseg = 0, ntseg = 0;
  for (int p = 0; p < n_prob; ++p) {
    CS_REQUIRE(h_qseg[p] >= 0 && h_tseg[p] >= 0, CS_ERR_INVALID,
               "cs_knn_feat: negative segment id in problem %d", p);
    nqseg = h_qseg[p] + 1 > nqseg ? h_qseg[p] + 1 : nqseg;
    ntseg = h_tseg[p] + 1 > ntseg ? h_tseg[p] + 1 : ntseg;
    const int64_t q0 = h_qoff[h_qseg[p]], t0 = h_toff[h_tseg[p]];
    int64_t qn = h_qoff[h_qseg[p] + 1] - q0, tn = h_toff[h_tseg[p] + 1] - t0;
    CS_REQUIRE(qn >= 0 && tn >= 0 && tn < (1LL << 31), CS_ERR_INVALID,
               "cs_knn_feat: bad segment in problem %d", p);
    for (int64_t q = 0; q < qn; q += qtile) {
      KnnWork w;
      w.q0 = q0 + q;
      w.t0 = t0;
      w.o0 = out_row + q;
      w.qn = (int32_t)(qn - q < qtile ? qn - q : qtile);
      w.tn = (int32_t)tn;
      w.prob = p;
      w.pad = h_tseg[p];  // target segment (label-order tables of the shortlist paths)
      work.push_back(w);
    }
    out_row += qn;
  }
  if (work.empty()) return CS_OK;
  PoolBuf<KnnWork> dwork;
  const int rc = upload(dwork, work, s);
  if (rc) return rc;
  double knn_flop = 0.0;
  for (const KnnWork& w : work) knn_flop += 3.0 * (double)w.qn * (double)w.tn * (double)dim;
  const KnnCall call = {d_qf, d_tf, h_qoff, h_toff, nqseg, ntseg, dim, k, d_qlabel, d_tlabel, d_perm, d_idx, d_dist,
                        dwork.p, (unsigned)work.size(), out_row, knn_flop, s};
  if (path == KnnOptions::F16) return knn_f16(call, opt);
  if (path == KnnOptions::F64) return knn_f64(call);
  return knn_exhaustive(call);
}

}  // extern "C"
