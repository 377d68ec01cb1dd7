// Hardest negatives of the metric-learning loop: for every anchor row of a query cloud the feature-nearest row
// of the problem's target cloud that is NOT a spatial neighbour of the anchor in the canonical frame (cs_hardest_negatives,
// include/corsair_hip.h is the specification).  FCGF trains its contrastive loss with such negatives; the reference ships
// pair lists and no loss.
// Every returned index / distance is that of the canonical f64 chain and of the exact f64 admissibility test.  The fast
// path only decides WHICH rows get the canonical evaluation:
//   * 16-d features (default): k_hn_classify finds every anchor's problem, a radix sort groups the anchors by problem,
//     k_hn_tiles cuts the groups into 256-anchor tiles, k_hn_f16 shortlists by |t|^2 - 2 q.t on the f16 matrix cores (the
//     hi / lo cut of nn_common.h) and runs the EXACT admissibility test on the values that pass a lane's threshold, so
//     only admissible rows ever enter a shortlist; k_hn_rescore evaluates the shortlist with the canonical chain and
//     accepts the winner only when it is vouched for (below); the rest goes through k_hn_exhaustive.
//   * CS_HARDNEG_MFMA=0 and every other width: k_hn_exhaustive for every anchor, one workgroup per anchor.
#include <hipcub/hipcub.hpp>

#include "nn_common.h"

namespace cs {

// one problem, as the kernels see it
struct HnProb {
  int64_t t0;   // first target row (row of d_tf / d_txyz)
  int32_t tn;   // target rows
  int32_t pad;
};

// one workgroup of k_hn_f16: 256 consecutive anchors (sorted order) of one problem
struct HnTile {
  int32_t a0;   // first position in the sorted anchor order
  int32_t an;   // anchors (0: unused tile)
  int32_t prob;
  int32_t pad;
};

constexpr int HN_NG = 2;        // 32-anchor groups per wave
constexpr int HN_QT = 4 * 32 * HN_NG;  // anchors per workgroup
constexpr int HN_KK = 4;        // shortlist per lane (two lanes per anchor): the winner is one row, the other entries are
                                // the slack between it and the threshold that vouches for it
constexpr int32_t HN_NONE = 0x7fffffff;
constexpr int HN_EX_GRID = 4096;   // workgroups of k_hn_exhaustive (16 per CU: enough to fill the device with one-anchor work)

// The scan is the shared one of nn_common.h (operand rows, stage, tile fragments, ranked list, error budget
// KNF_EPS_REL (|q|^2 + |t|^2_max)); this unit adds an ABSOLUTE term to the budget, because mined features need not be
// unit vectors: below f16's normal range the hi + lo cut leaves a residue of up to 2^-25 per component, in the value at
// most 2^-25 (|a|_1 + |b|_1) <= 2^-22 (|q| + |t|) with a = -2 q, b = t (|x|_1 <= 4 |x|_2 in 16-d); charged
// HN_EPS_ABS (|q| + |t|_max).
constexpr double HN_EPS_ABS = 0x1.0p-20;

// problem of every anchor (binary search of its row in the query offsets), sort key = problem (n_prob: in no problem;
// such anchors are answered here: -1 / +inf)
__global__ void k_hn_classify(const int32_t* __restrict__ anchor, int64_t A, const int64_t* __restrict__ qoff, int nqseg,
                              const int32_t* __restrict__ seg2prob, int n_prob, uint32_t* __restrict__ keys,
                              int32_t* __restrict__ vals, int32_t* __restrict__ out_idx, double* __restrict__ out_dist) {
  const int64_t a = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (a >= A) return;
  const int64_t row = anchor[a];
  int prob = -1;
  if (nqseg > 0 && row >= qoff[0] && row < qoff[nqseg]) {
    int lo = 0, hi = nqseg;  // last segment with qoff[s] <= row (empty segments share an offset: the last one holds the row)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (qoff[mid] <= row) lo = mid; else hi = mid;
    }
    prob = seg2prob[lo];
  }
  keys[a] = prob >= 0 ? (uint32_t)prob : (uint32_t)n_prob;
  vals[a] = (int32_t)a;
  if (prob < 0) {
    out_idx[a] = -1;
    if (out_dist) out_dist[a] = INFINITY;
  }
}

// tiles of the sorted anchor order: problem p owns the positions [first key >= p, first key >= p + 1).  One workgroup;
// the tile table was zeroed before (unused tiles have an = 0).  One thread writes the table: A / 256 + n_prob entries of
// 16 B, 160 at the training size (a few microseconds); a scan over the problems' tile counts would make it parallel and
// was not built.
__global__ void k_hn_tiles(const uint32_t* __restrict__ keys_sorted, int64_t A, int n_prob, int32_t* __restrict__ pstart,
                           HnTile* __restrict__ tiles) {
  for (int p = threadIdx.x; p <= n_prob; p += blockDim.x) {
    int64_t lo = 0, hi = A;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (keys_sorted[mid] < (uint32_t)p) lo = mid + 1; else hi = mid;
    }
    pstart[p] = (int32_t)lo;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int n = 0;
  for (int p = 0; p < n_prob; ++p)
    for (int a = pstart[p]; a < pstart[p + 1]; a += HN_QT) {
      HnTile t;
      t.a0 = a;
      t.an = min(HN_QT, pstart[p + 1] - a);
      t.prob = p;
      t.pad = 0;
      tiles[n++] = t;
    }
}

// target image (row j of the image = row j of d_tf): [th(16) | tl(16) | th(16) | 0(8)]; t4 = {x, y, z, |t|^2 (f64 chain,
// to f32)}; seg_t2max[seg] = max |t|^2 rounded up (unsigned maximum of the bit patterns of non-negative floats: an integer
// atomic, the same in any order)
__global__ void k_hn_pack_targets(const float* __restrict__ tf, int ld, const float* __restrict__ txyz,
                                  const int64_t* __restrict__ toff, _Float16* __restrict__ img,
                                  float4* __restrict__ t4, unsigned* __restrict__ seg_t2max_bits) {
  const int sg = blockIdx.y;
  const int64_t b = toff[sg], e = toff[sg + 1];
  float mx = 0.f;
  for (int64_t j = b + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < e; j += (int64_t)gridDim.x * blockDim.x) {
    const double n2 = knf_pack_target_row(tf + j * ld, img + j * KNF_PITCH);
    t4[j] = make_float4(txyz[3 * j], txyz[3 * j + 1], txyz[3 * j + 2], (float)n2);
    mx = fmaxf(mx, (float)n2 * 1.0000002f);
  }
  knf_seg_max(mx, &seg_t2max_bits[sg]);
}

// anchor operand rows in sorted order: [-2 qh(16) | -2 qh(16) | -2 ql(16)] (the scaling by 2 is exact), q4 = {x, y, z, 0}
__global__ void k_hn_pack_anchors(const float* __restrict__ qf, int ld, const float* __restrict__ qxyz,
                                  const int32_t* __restrict__ anchor, const uint32_t* __restrict__ keys_sorted,
                                  const int32_t* __restrict__ vals_sorted, int64_t A, int n_prob,
                                  _Float16* __restrict__ qrows, float4* __restrict__ q4) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= A || keys_sorted[i] >= (uint32_t)n_prob) return;
  const int64_t r = anchor[vals_sorted[i]];
  knf_pack_query_row(qf + r * ld, qrows + i * 48);
  q4[i] = make_float4(qxyz[3 * r], qxyz[3 * r + 1], qxyz[3 * r + 2], 0.f);
}

// ------------------------------------------------------------------------------------------
// The shortlist scan.  rows = targets (LDS, staged by LDS-DMA from the 112-B-pitch f16 image), cols = anchors (registers):
// a lane owns one anchor and 16 of a tile's 32 target rows, the two lanes of an anchor (lane, lane ^ 32) own disjoint
// halves.  A value below the lane's threshold is a HIT: only then the exact f64 admissibility test of (anchor, row) runs,
// on the f32 points staged beside the image, and only an admissible row enters the lane's list (the HN_KK smallest
// approximate values, ascending).  The threshold is the smaller of the two lanes' HN_KK-th values and never rises.
// What the lists guarantee at the end (tau = final threshold): a row that is in neither list is inadmissible (tested
// exactly), or its approximate value was >= the threshold of its time >= tau, or it was displaced from a full list by
// smaller values, so it is >= that list's HN_KK-th value >= tau.  tau = +inf: no list ever filled, every admissible row of
// the segment is in a list.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hn_f16(const HnTile* __restrict__ tiles, const HnProb* __restrict__ probs,
                                                const _Float16* __restrict__ qrows, const float4* __restrict__ q4,
                                                const _Float16* __restrict__ img, const float4* __restrict__ t4,
                                                double r2, int use_excl, int32_t* __restrict__ cand_i,
                                                float* __restrict__ cand_tau) {
  constexpr int STAGE_BYTES = KNF_STAGE_BYTES;
  __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE_BYTES];
  __shared__ __attribute__((aligned(16))) float tn_s[2][KNF_ROWS];
  __shared__ __attribute__((aligned(16))) float4 x_s[2][KNF_ROWS];
  const HnTile tile = tiles[blockIdx.x];
  if (tile.an == 0) return;  // (block-uniform)
  const HnProb pb = probs[tile.prob];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5;
  const int col = lane & 31;
  f16x8 bop[HN_NG][3];
  double qx[HN_NG], qy[HN_NG], qz[HN_NG];
  bool qvalid[HN_NG];
  float bd[HN_NG][HN_KK], thr[HN_NG];
  int32_t bi[HN_NG][HN_KK];
#pragma unroll
  for (int g = 0; g < HN_NG; ++g) {
    const int qloc = wave * 32 * HN_NG + 32 * g + col;
    qvalid[g] = qloc < tile.an;
    const int64_t qpos = tile.a0 + (qvalid[g] ? qloc : 0);
    const _Float16* row = qrows + qpos * 48 + 8 * half;
#pragma unroll
    for (int m = 0; m < 3; ++m) bop[g][m] = *reinterpret_cast<const f16x8*>(row + 16 * m);
    const float4 p = q4[qpos];
    qx[g] = (double)p.x;
    qy[g] = (double)p.y;
    qz[g] = (double)p.z;
    thr[g] = INFINITY;
#pragma unroll
    for (int j = 0; j < HN_KK; ++j) {
      bd[g][j] = INFINITY;
      bi[g][j] = HN_NONE;
    }
  }
  const int t_hi = pb.tn;
  if (t_hi > 0) {
    const char* gimg = reinterpret_cast<const char*>(img + pb.t0 * KNF_PITCH) + lane * 16;
    const unsigned lds_base = __builtin_amdgcn_readfirstlane(lds_addr_of(lds));
    // (LDS-DMA as inline asm, the points and |t|^2 loaded before it and stored after the stage's compute: common.h)
    auto issue_dma = [&](int b, int base) { knf_issue_dma(gimg, lds_base, wave, b, base); };
    auto load_rows = [&](int base, float4& v) {   // unconditional (clamped) load
      int r = base + (tid % KNF_ROWS);
      r = r > t_hi - 1 ? t_hi - 1 : r;
      v = t4[pb.t0 + r];
    };
    auto store_rows = [&](int b, int base, const float4& v) {
      if (tid < KNF_ROWS) {
        tn_s[b][tid] = base + tid < t_hi ? v.w : INFINITY;   // rows past the segment can never be hit
        x_s[b][tid] = v;
      }
    };
    {
      float4 v0;
      load_rows(0, v0);
      issue_dma(0, 0);
      store_rows(0, 0, v0);
    }
    int buf = 0;
    for (int base = 0; base < t_hi; base += KNF_ROWS) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      const bool more = base + KNF_ROWS < t_hi;
      float4 v_next;
      load_rows(base + KNF_ROWS, v_next);
      if (more) issue_dma(buf ^ 1, base + KNF_ROWS);
#pragma unroll 1
      for (int t = 0; t < KNF_ROWS / 32; ++t) {
        if (base + 32 * t >= t_hi) break;  // whole tile past the segment (block-uniform)
        f16x8 a[3];
        f32x16 c16;
        knf_load_tile(lds + buf * STAGE_BYTES, tn_s[buf], t, col, half, a, c16);
#pragma unroll
        for (int g = 0; g < HN_NG; ++g) {
          f32x16 d = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[0], bop[g][0], c16, 0, 0, 0);
          d = knf_mfma_lo(a, bop[g], d);
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool hit = d[r] < thr[g];
            if (__any(hit)) {
              if (hit) {
                const int srow = knf_result_row(t, half, r);   // row of the stage
                bool adm = true;
                if (use_excl) {
                  const float4 p = x_s[buf][srow];
                  const double dx = qx[g] - (double)p.x, dy = qy[g] - (double)p.y, dz = qz[g] - (double)p.z;
                  adm = !(((dx * dx + dy * dy) + dz * dz) < r2);
                }
                if (adm) knf_insert(bd[g], bi[g], d[r], base + srow);   // (row local to the target segment)
              }
              thr[g] = fminf(thr[g], knf_pair_min(bd[g][HN_KK - 1]));
            }
          }
        }
      }
      if (more) store_rows(buf ^ 1, base + KNF_ROWS, v_next);
      buf ^= 1;
    }
  }
#pragma unroll
  for (int g = 0; g < HN_NG; ++g) {
    const int qloc = wave * 32 * HN_NG + 32 * g + col;
    if (qvalid[g]) {
      const int64_t qpos = tile.a0 + qloc;
#pragma unroll
      for (int j = 0; j < HN_KK; ++j) cand_i[(qpos * 2 + half) * HN_KK + j] = bi[g][j];
      if (half == 0) cand_tau[qpos] = thr[g];
    }
  }
}

// One thread per anchor (sorted order): canonical distances of its 2 * HN_KK shortlisted rows -- admissible already, the
// scan tested them exactly --, winner by (distance, row), and the VOUCHER: every row outside the lists is inadmissible or
// has an approximate value >= tau, hence an exact d - |q|^2 >= tau - eps.  The winner stands iff its own d - |q|^2 is
// strictly below tau - eps: a row that merely ties with it (where the smaller index would decide) cannot be vouched for and
// sends the anchor to k_hn_exhaustive, as does everything outside the f16 range.  tau = +inf: nothing was left out (an empty
// list then means that no row is admissible: -1).
__global__ void k_hn_rescore(const float* __restrict__ qf, int ld_q, const float* __restrict__ tf, int ld_t,
                             const int32_t* __restrict__ anchor, const uint32_t* __restrict__ keys_sorted,
                             const int32_t* __restrict__ vals_sorted, int64_t A, int n_prob,
                             const HnProb* __restrict__ probs, const int32_t* __restrict__ prob_tseg,
                             const int32_t* __restrict__ cand_i, const float* __restrict__ cand_tau,
                             const unsigned* __restrict__ seg_t2max_bits, int32_t* __restrict__ out_idx,
                             double* __restrict__ out_dist, int32_t* __restrict__ flag) {
  const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  if (i >= A) return;
  const uint32_t p = keys_sorted[i];
  if (p >= (uint32_t)n_prob) return;   // in no problem: answered by k_hn_classify (flag stays 0)
  const int32_t a = vals_sorted[i];
  const float* qp = qf + (int64_t)anchor[a] * ld_q;
  const HnProb pb = probs[p];
  double q[16], qn2 = 0.0;
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    q[c] = (double)qp[c];
    qn2 = fma(q[c], q[c], qn2);
  }
  double bd = INFINITY;
  int32_t br = HN_NONE;
  for (int c = 0; c < 2 * HN_KK; ++c) {
    const int32_t row = cand_i[i * 2 * HN_KK + c];
    if (row == HN_NONE) continue;
    const double d = knf_chain16(q, tf + (pb.t0 + row) * ld_t);
    if (d < bd || (d == bd && row < br)) {
      bd = d;
      br = row;
    }
  }
  const float tau = cand_tau[i];
  const double t2max = (double)__uint_as_float(seg_t2max_bits[prob_tseg[p]]);
  bool ok = true;
  if (tau < INFINITY) {
    const double eps = KNF_EPS_REL * (qn2 + t2max) + HN_EPS_ABS * (sqrt(qn2) + sqrt(t2max));
    ok = br != HN_NONE && (bd - qn2) < (double)tau - eps;
  }
  if (!(tau == tau) || !(qn2 < KNF_RANGE) || !(t2max < KNF_RANGE)) ok = false;
  flag[i] = ok ? 0 : 1;
  if (ok) {
    out_idx[a] = br != HN_NONE ? br : -1;
    if (out_dist) out_dist[a] = br != HN_NONE ? sqrt(bd) : INFINITY;
  }
}

// ------------------------------------------------------------------------------------------
// Exhaustive search, any width: one workgroup per anchor (sorted order), thread t takes the target rows t, t + 256, ...:
// exact admissibility, canonical chain, the thread's best by (distance, row); the 256 bests are reduced by the same order,
// so the result does not depend on which thread saw which row.  flag != nullptr: only the anchors the voucher refused.
// The grid is fixed (HN_EX_GRID workgroups at most) and a workgroup strides over the anchors: in the fallback launch nearly
// every anchor is unflagged, and a workgroup skips eight of them for the price of eight loads instead of the library
// launching one empty workgroup per anchor.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hn_exhaustive(const float* __restrict__ qf, int ld_q,
                                                       const float* __restrict__ qxyz, const float* __restrict__ tf,
                                                       int ld_t, const float* __restrict__ txyz, int C,
                                                       const int32_t* __restrict__ anchor,
                                                       const uint32_t* __restrict__ keys_sorted,
                                                       const int32_t* __restrict__ vals_sorted, int64_t A,
                                                       int n_prob, const HnProb* __restrict__ probs, double r2,
                                                       int use_excl,
                                                       const int32_t* __restrict__ flag, int32_t* __restrict__ out_idx,
                                                       double* __restrict__ out_dist) {
  __shared__ double q_s[256];
  __shared__ double rd_s[256];
  __shared__ int32_t ri_s[256];
  for (int64_t i = blockIdx.x; i < A; i += gridDim.x) {   // (every condition below is uniform in the workgroup)
  if (flag && !flag[i]) continue;
  const uint32_t p = keys_sorted[i];
  if (p >= (uint32_t)n_prob) continue;
  const int32_t a = vals_sorted[i];
  const int64_t qrow = anchor[a];
  const HnProb pb = probs[p];
  const int tid = threadIdx.x;
  if (tid < C) q_s[tid] = (double)qf[qrow * ld_q + tid];
  __syncthreads();
  const double qx = (double)qxyz[3 * qrow], qy = (double)qxyz[3 * qrow + 1], qz = (double)qxyz[3 * qrow + 2];
  double bd = INFINITY;
  int32_t br = HN_NONE;
  for (int j = tid; j < pb.tn; j += 256) {
    const int64_t trow = pb.t0 + j;
    if (use_excl) {
      const double dx = qx - (double)txyz[3 * trow], dy = qy - (double)txyz[3 * trow + 1],
                   dz = qz - (double)txyz[3 * trow + 2];
      if (((dx * dx + dy * dy) + dz * dz) < r2) continue;
    }
    const float* tp = tf + trow * ld_t;
    double d = 0.0;
    for (int c = 0; c < C; ++c) {
      const double diff = q_s[c] - (double)tp[c];
      d = fma(diff, diff, d);
    }
    if (d < bd) {   // rows ascend within a thread: strict < keeps the smaller row
      bd = d;
      br = j;
    }
  }
  rd_s[tid] = bd;
  ri_s[tid] = br;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) {
      const double od = rd_s[tid + w];
      const int32_t oi = ri_s[tid + w];
      if (oi != HN_NONE && (ri_s[tid] == HN_NONE || od < rd_s[tid] || (od == rd_s[tid] && oi < ri_s[tid]))) {
        rd_s[tid] = od;
        ri_s[tid] = oi;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const bool have = ri_s[0] != HN_NONE;
    out_idx[a] = have ? ri_s[0] : -1;
    if (out_dist) out_dist[a] = have ? sqrt(rd_s[0]) : INFINITY;
  }
  __syncthreads();   // q_s / rd_s / ri_s are reused by the next anchor
  }
}

}  // namespace cs

using namespace cs;

// {anchors answered, of those recomputed exhaustively}; counted only while CS_HARDNEG_STATS=1 (the count synchronises)
static std::atomic<unsigned long long> g_hn_stats[2];

extern "C" {

void cs_hardest_stats(uint64_t out[2], int reset) { read_stats(g_hn_stats, out, reset); }

int cs_hardest_negatives(const float* d_qf, int ld_q, const float* d_qxyz, const int64_t* h_qoff, const float* d_tf,
                         int ld_t, const float* d_txyz, const int64_t* h_toff, const int32_t* h_qseg,
                         const int32_t* h_tseg, int n_prob, int C, const int32_t* d_anchor, int64_t A, double radius,
                         int32_t* d_idx, double* d_dist, void* stream) {
  CS_REQUIRE(n_prob >= 0 && A >= 0, CS_ERR_INVALID, "cs_hardest_negatives: negative count");
  CS_REQUIRE(A < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_hardest_negatives: too many anchors");
  CS_REQUIRE(C >= 1 && C <= 256, CS_ERR_UNSUPPORTED, "cs_hardest_negatives: width %d not in [1, 256]", C);
  CS_REQUIRE(ld_q >= C && ld_t >= C, CS_ERR_INVALID, "cs_hardest_negatives: leading dimension below the width");
  CS_REQUIRE(n_prob == 0 || (h_qoff && h_toff && h_qseg && h_tseg), CS_ERR_INVALID,
             "cs_hardest_negatives: NULL segment table");
  CS_REQUIRE(A == 0 || (d_anchor && d_idx), CS_ERR_INVALID, "cs_hardest_negatives: NULL anchors or output");
  CS_REQUIRE(A == 0 || n_prob == 0 || (d_qf && d_tf && d_qxyz && d_txyz), CS_ERR_INVALID,
             "cs_hardest_negatives: NULL features or points");
  CS_REQUIRE(radius == radius, CS_ERR_INVALID, "cs_hardest_negatives: radius is not a number");
  int nqseg = 0, ntseg = 0;
  for (int p = 0; p < n_prob; ++p) {
    CS_REQUIRE(h_qseg[p] >= 0 && h_tseg[p] >= 0, CS_ERR_INVALID,
               "cs_hardest_negatives: negative segment id in problem %d", p);
    nqseg = h_qseg[p] + 1 > nqseg ? h_qseg[p] + 1 : nqseg;
    ntseg = h_tseg[p] + 1 > ntseg ? h_tseg[p] + 1 : ntseg;
  }
  std::vector<int32_t> seg2prob((size_t)nqseg, -1), prob_tseg((size_t)n_prob);
  std::vector<HnProb> probs((size_t)n_prob);
  for (int s = 0; s < nqseg; ++s)
    CS_REQUIRE(h_qoff[s] >= 0 && h_qoff[s + 1] >= h_qoff[s], CS_ERR_INVALID,
               "cs_hardest_negatives: query offsets do not ascend at %d", s);
  for (int s = 0; s < ntseg; ++s)
    CS_REQUIRE(h_toff[s] >= 0 && h_toff[s + 1] >= h_toff[s], CS_ERR_INVALID,
               "cs_hardest_negatives: target offsets do not ascend at %d", s);
  double flop = 0.0;
  for (int p = 0; p < n_prob; ++p) {
    CS_REQUIRE(seg2prob[h_qseg[p]] < 0, CS_ERR_INVALID,
               "cs_hardest_negatives: query segment %d is in problems %d and %d (an anchor has one problem)", h_qseg[p],
               seg2prob[h_qseg[p]], p);
    seg2prob[h_qseg[p]] = p;
    const int64_t tn = h_toff[h_tseg[p] + 1] - h_toff[h_tseg[p]];
    CS_REQUIRE(tn < (1LL << 31), CS_ERR_UNSUPPORTED, "cs_hardest_negatives: target segment of problem %d too long", p);
    probs[p].t0 = h_toff[h_tseg[p]];
    probs[p].tn = (int32_t)tn;
    probs[p].pad = 0;
    prob_tseg[p] = h_tseg[p];
  }
  const int64_t nt_rows = ntseg ? h_toff[ntseg] : 0;
  CS_REQUIRE(nt_rows < (1LL << 31) && (nqseg ? h_qoff[nqseg] : 0) < (1LL << 31), CS_ERR_UNSUPPORTED,
             "cs_hardest_negatives: too many rows");
  if (A == 0) return CS_OK;
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const bool use_f16 = C == 16 && !env_first_is("CS_HARDNEG_MFMA", '0');
  const bool stats = env_first_is("CS_HARDNEG_STATS", '1');
  const int use_excl = radius > 0.0 ? 1 : 0;
  const double r2 = radius * radius;

  // every anchor's problem, the anchors grouped by problem: all on the stream, the host never sees an anchor
  PoolBuf<int64_t> dqoff;
  PoolBuf<int32_t> dseg2prob, dprob_tseg, vals, vals_sorted;
  PoolBuf<HnProb> dprobs;
  PoolBuf<uint32_t> keys, keys_sorted;
  PoolBuf<char> tmp;
  std::vector<int64_t> qoff(h_qoff ? h_qoff : nullptr, h_qoff ? h_qoff + (n_prob ? nqseg + 1 : 0) : nullptr);
  int rc = upload(dqoff, qoff, s);
  if (!rc) rc = upload(dseg2prob, seg2prob, s);
  if (!rc) rc = upload(dprobs, probs, s);
  if (!rc) rc = upload(dprob_tseg, prob_tseg, s);
  if (rc) return rc;
  CS_REQUIRE(keys.alloc((size_t)A) && keys_sorted.alloc((size_t)A) && vals.alloc((size_t)A) &&
                 vals_sorted.alloc((size_t)A),
             CS_ERR_HIP, "cs_hardest_negatives: scratch allocation failed");
  const double units = 2.0 * (double)C;  // per (anchor, target row); the anchors' shares are not known on the host
  for (int p = 0; p < n_prob; ++p) flop += units * (double)probs[p].tn;
  if (n_prob) flop *= (double)A / (double)n_prob;   // (anchors spread evenly over the problems: the profile's work figure only)
  const dim3 ex_grid((unsigned)(A < HN_EX_GRID ? A : HN_EX_GRID));
  ProfScope prof("hardneg", s, flop);   // the whole call: classify, sort, tiles, packs, scan, re-score, fallback
  hipLaunchKernelGGL(k_hn_classify, dim3((unsigned)ceil_div(A, 256)), dim3(256), 0, s, d_anchor, A, dqoff.p, nqseg,
                     dseg2prob.p, n_prob, keys.p, vals.p, d_idx, d_dist);
  CS_LAUNCH_CHECK();
  if (n_prob == 0) return CS_OK;
  int end_bit = 1;
  while ((1LL << end_bit) <= (int64_t)n_prob) ++end_bit;
  size_t tmp_bytes = 0;
  CS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, keys.p, keys_sorted.p, vals.p, vals_sorted.p,
                                                  (int)A, 0, end_bit, s));
  CS_REQUIRE(tmp.alloc(tmp_bytes ? tmp_bytes : 1), CS_ERR_HIP, "cs_hardest_negatives: scratch allocation failed");
  CS_HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, keys.p, keys_sorted.p, vals.p, vals_sorted.p, (int)A,
                                                  0, end_bit, s));

  if (!use_f16) {
    hipLaunchKernelGGL(k_hn_exhaustive, ex_grid, dim3(256), 0, s, d_qf, ld_q, d_qxyz, d_tf, ld_t, d_txyz, C,
                       d_anchor, keys_sorted.p, vals_sorted.p, A, n_prob, dprobs.p, r2, use_excl, (const int32_t*)nullptr,
                       d_idx, d_dist);
    CS_LAUNCH_CHECK();
    if (stats) {
      g_hn_stats[0] += (unsigned long long)A;
      g_hn_stats[1] += (unsigned long long)A;
    }
    return CS_OK;
  }

  const unsigned n_tile = (unsigned)(ceil_div(A, HN_QT) + n_prob);   // sum_p ceil(a_p / 256) is at most that
  PoolBuf<HnTile> tiles((size_t)n_tile);
  PoolBuf<int32_t> pstart((size_t)n_prob + 1), cand((size_t)A * 2 * HN_KK), flag((size_t)A);
  PoolBuf<_Float16> qrows((size_t)A * 48), img((size_t)(nt_rows + KNF_ROWS) * KNF_PITCH);  // + one stage of slack
  PoolBuf<float4> q4((size_t)A), t4((size_t)(nt_rows ? nt_rows : 1));
  PoolBuf<float> tau((size_t)A);
  PoolBuf<unsigned> t2max((size_t)ntseg);
  PoolBuf<int64_t> dtoff;
  CS_REQUIRE(tiles.p && pstart.p && cand.p && flag.p && qrows.p && img.p && q4.p && t4.p && tau.p && t2max.p, CS_ERR_HIP,
             "cs_hardest_negatives: scratch allocation failed");
  std::vector<int64_t> toff(h_toff, h_toff + ntseg + 1);
  rc = upload(dtoff, toff, s);
  if (rc) return rc;
  CS_HIP_CHECK(hipMemsetAsync(tiles.p, 0, sizeof(HnTile) * n_tile, s));
  CS_HIP_CHECK(hipMemsetAsync(t2max.p, 0, sizeof(unsigned) * ntseg, s));
  CS_HIP_CHECK(hipMemsetAsync(flag.p, 0, sizeof(int32_t) * (size_t)A, s));
  hipLaunchKernelGGL(k_hn_tiles, dim3(1), dim3(256), 0, s, keys_sorted.p, A, n_prob, pstart.p, tiles.p);
  CS_LAUNCH_CHECK();
  if (nt_rows) {
    hipLaunchKernelGGL(k_hn_pack_targets, dim3(16, (unsigned)ntseg), dim3(256), 0, s, d_tf, ld_t, d_txyz, dtoff.p, img.p,
                       t4.p, t2max.p);
    CS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_hn_pack_anchors, dim3((unsigned)ceil_div(A, 256)), dim3(256), 0, s, d_qf, ld_q, d_qxyz, d_anchor,
                     keys_sorted.p, vals_sorted.p, A, n_prob, qrows.p, q4.p);
  CS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hn_f16, dim3(n_tile), dim3(256), 0, s, tiles.p, dprobs.p, qrows.p, q4.p, img.p, t4.p, r2, use_excl,
                     cand.p, tau.p);
  CS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_hn_rescore, dim3((unsigned)ceil_div(A, 256)), dim3(256), 0, s, d_qf, ld_q, d_tf, ld_t, d_anchor,
                     keys_sorted.p, vals_sorted.p, A, n_prob, dprobs.p, dprob_tseg.p, cand.p, tau.p, t2max.p, d_idx,
                     d_dist, flag.p);
  CS_LAUNCH_CHECK();
  // exhaustive recomputation of the anchors whose winner could not be vouched for
  hipLaunchKernelGGL(k_hn_exhaustive, ex_grid, dim3(256), 0, s, d_qf, ld_q, d_qxyz, d_tf, ld_t, d_txyz, C, d_anchor,
                     keys_sorted.p, vals_sorted.p, A, n_prob, dprobs.p, r2, use_excl, flag.p, d_idx, d_dist);
  CS_LAUNCH_CHECK();
  if (stats) {
    unsigned long long h = 0;
    rc = count_flagged(flag.p, A, &h, s, "cs_hardest_negatives");
    if (rc) return rc;
    g_hn_stats[0] += (unsigned long long)A;
    g_hn_stats[1] += h;
  }
  return CS_OK;
}

}  // extern "C"
