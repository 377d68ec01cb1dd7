// Feature k-NN shortlist on the f16 matrix cores (16-d features, k <= 6): the default path of cs_knn_feat (knn.hip).
// On gfx950 an f64 MFMA runs on the vector unit's double-precision ALUs (78.6 TF either way) and cannot overlap
// with the VALU work that ranks its results.  Here |t|^2 - 2 q.t is evaluated like the RANSAC prefilter: every
// feature is split into f16 hi + lo, hi*hi + lo*hi + hi*lo (48 products) is three v_mfma_f32_32x32x16_f16 per
// 32 x 32 tile (true matrix cores, ~20x the f64 rate, co-issuing with the VALU), the accumulator is preloaded with |t|^2.
//   rows = targets (LDS, staged by LDS-DMA from a 112-B-pitch f16 image in visiting order),
//   cols = queries (registers): a lane owns one query and 16 of the tile's 32 target rows.
// The result is only a SHORTLIST (2 x KNF_KK candidates per query by the approximate value).
// k_knn_rescore_f16 re-evaluates them with the canonical f64 chain, ranks by (distance, row) and
// VERIFIES the shortlist: every target that was not kept has an approximate value >= tau (the final
// pruning threshold), hence an exact one >= tau - eps; if the exact k-th distance is not below that,
// the query is flagged and recomputed by the exhaustive kernel (k_knn_feat<16>, knn_exact.hip; flagged tiles only).
// The answer therefore equals the exhaustive kernel's for every query.
// Labelled searches (part-to-part correspondences): the targets of a segment are visited in label order (label_order:
// k_seg_keys, a radix sort, k_label_starts) and a workgroup scans only the rows of the labels it wants.
#include <hipcub/hipcub.hpp>

#include "knn.h"

namespace cs {

// (KNF_PITCH, KNF_ROWS, the operand rows, the stage and tile helpers and the error budget: nn_common.h, shared with
// hardneg.hip; KNF_KK: knn.h)
constexpr int KNF_NG = 2;       // 32-query groups per wave
constexpr int KNF_QT = 4 * 32 * KNF_NG;  // queries per workgroup
static_assert(KNF_QT == 256, "tiles of the f16 path and of the exhaustive fallback must coincide");
constexpr int KNF_PEND = 4;

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
  // Ranked shortlist (ascending) plus a small unranked pending list per lane and group.  A candidate below the lane's
  // threshold is only appended (a register shift); the pending lists of the whole wave are ranked together when one of
  // them is full.  Ranking on every hit would run the 8-slot insertion for nearly every element, because some lane of
  // the 64 almost always has a hit.
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
// the verification of the shortlist (see the header of this file).  flag[tile] != 0 -> k_knn_feat
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

// f16 matrix-core shortlist (k_knn_f16), canonical rescore and verification (k_knn_rescore_f16), exhaustive recomputation
// of the queries that fail it (knn_exact_launch, flagged tiles only)
int knn_f16(const KnnCall& c, const KnnOptions& opt, unsigned long long* n_redone) {
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
    knn_exact_launch(c, tile_flag.p, qflag.p);
    CS_LAUNCH_CHECK();
  }
  if (opt.stats && out_row > 0) return count_flagged(qflag.p, out_row, n_redone, s, "cs_knn_feat");
  return CS_OK;
}

}  // namespace cs
