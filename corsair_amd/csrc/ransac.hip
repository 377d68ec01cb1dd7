// Batched correspondence RANSAC on gfx950.
//
// Replaces registration_based_on_corr -> Open3D registration_ransac_based_on_correspondence
// (utils/eval_pose.py:82-100 of the reference; ransac_n = 10, 100 000 iterations, confidence 0.999).
// Semantics: Open3D's loop as executed by ONE thread (iteration order = index order), with the
// global Mersenne twister replaced by a counter-based generator so that iteration i of every
// problem is reproducible anywhere.  Iterations are processed in rounds of growing chunks: [0, 64) (CS_RANSAC_FIRST),
// [64, 512), then doubling -- [512, 1024), [1024, 2048), ... -- up to 16 384 per round.  The first chunk is counted
// exactly (there is no best count to prune against yet); every later one goes through the f16 prefilter.
// Non-finite pairs (include/corsair_hip.h): a pair with a NaN or infinite coordinate is never an inlier (`d2 < thr2` is
// false in every exact kernel) and puts its problem's largest point norm out of the f16 range, so that problem bypasses
// the prefilter (ransac_prefilter.hip: smax) and every one of its hypotheses is counted exactly; a hypothesis fitted to
// such a pair has no inliers, and k_ransac_scan1 takes a best only from a count above zero.
// The kernels live in four units that share ransac.h (state, constants, launch functions): this one holds the sequential
// replay (k_ransac_scan1, k_ransac_scan2, k_ransac_finish) and the host driver.  A round:
//   k_ransac_hyp        (ransac_hyp.hip) one lane per hypothesis: sample ransac_n pairs (packed 32-B rows), closed-form
//                       rigid fit (Horn quaternion; largest eigenpair of the 4x4 matrix from its characteristic
//                       polynomial, horn_qcp, with the Jacobi eigen-solver as per-lane fallback; f64), emit R|t as f64
//                       (Open3D keeps the Matrix4d; the f32 cast happens at the very end, where the
//                       reference casts the result: utils/symmetry.py:274); in a prefiltered round also the
//                       hypothesis' prefilter row (pf_emit_row: 16 f16 coefficients + c_h)
//   k_ransac_prefilter  (ransac_prefilter.hip; from the second chunk on) an UPPER bound of every hypothesis' inlier count on the
//                       f16 matrix cores; hypotheses whose bound is below the carried best cannot
//                       matter and get count 0.  <1, true> = one MFMA per tile (K = 16: a_hi . b_hi',
//                       the dropped term bounded per pair), signs counted by v_add_f32 under
//                       round-toward-minus-infinity; 0.2 % survive.  <2, false> = two MFMAs per tile (K = 32:
//                       a_hi . (b_hi + b_lo)), signs through a v_alignbit history: the whole prefilter with
//                       CS_RANSAC_PF_K=32, and always the SECOND STAGE -- the survivors of the K = 16 bound,
//                       compacted by k_ransac_survivors, go through it (list mode) before the exact count.  See the
//                       block comments above k_ransac_pack16_b0 / the kernel there and DESIGN.md ("RANSAC prefilter").
//   k_ransac_count      (ransac_count.hip) the exact count in Open3D's arithmetic: the reference hands Open3D f64 points
//                       (utils/eval_pose.py:83-86) and Eigen transforms and compares in double, so the
//                       inlier test is evaluated in f64: a lane owns one hypothesis (R|t in 12 f64
//                       registers), the pairs of a 256-row stage are converted to f64 once and read
//                       from LDS as broadcasts; p = fma(r2,sz, fma(r1,sy, fma(r0,sx, t))), d = p - q,
//                       |d|^2 = fma(dz,dz, fma(dy,dy, dx dx)) < max_corr^2 (the canonical chain, the
//                       oracle's).  Used for all hypotheses of an unfiltered chunk (<false, 64> for a chunk of 64)
//                       and (<true>) for survivor lists longer than 1024 per problem; k_ransac_count_few handles
//                       the usual handful of survivors (same chain, count and fixed-point error in one pass).  These
//                       kernels see ~0.1 % of the (hypothesis, pair) work; the f16 prefilter carries the rest.
//   k_ransac_scan1      (here) one wave per problem replays the chunk in iteration order (prefix max of the
//                       inlier counts -> early-exit bound est_k -> stop position) and lists the
//                       hypotheses that tie for the best count.  When k_ransac_count_few has left their errors it
//                       also picks the best of them: the usual round is hyp -> prefilter -> survivors ->
//                       second-stage prefilter -> count_few -> scan1, six launches.  Otherwise:
//   k_ransac_err        (ransac_count.hip) fixed-point squared error (exact integer sums) of those few candidates
//   k_ransac_scan2      (here) best = max count, then min error, then first -- the final state of the
//                       sequential rule "better = more inliers, or equal inliers and smaller rmse"
// The host loop (cs_ransac_batch, at the end of this file) synchronises once per round (one pinned copy of the
// per-problem state); the next round's hypotheses and prefilter are already enqueued at that point.
// Inlier counts and fixed-point errors are integers, so any split of the correspondence range across
// workgroups gives identical sums.
#include <math.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "ransac.h"

namespace cs {

// est_k implied by a best inlier count c (Open3D: log(1 - confidence) / log(1 - ratio^n))
__device__ __forceinline__ int est_bound(int c, int m, int ransac_n, double log_1mc, int est_k0) {
  const double ratio = fmin(1.0, (double)c / (double)m);
  double pw = 1.0;
  for (int j = 0; j < ransac_n; ++j) pw = pw * ratio;
  const double den = log(1.0 - pw);
  if (den < 0.0) {  // den == 0: (inliers/M)^n below 2^-53 -> no finite bound
    const double est = log_1mc / den;
    if (est < (double)est_k0) return (int)ceil(est);
  }
  return est_k0;
}

// One wave per problem: sequential-semantics replay of the chunk from the inlier counts alone.
__global__ __launch_bounds__(256) void k_ransac_scan1(RansacProb* probs, int n_prob,
                                                     const int32_t* __restrict__ res_cnt, int it0,
                                                     int bcount, int bmax, int ransac_n,
                                                     int max_iter, double log_1mc,
                                                     int32_t* __restrict__ cand, int* n_active,
                                                     // fused k_ransac_scan2 (err_by_h != nullptr: k_ransac_count_few left the
                                                     // error of every survivor, so no k_ransac_err has to run in between)
                                                     const unsigned long long* __restrict__ err_by_h,
                                                     const double* __restrict__ hyp, int32_t* __restrict__ next_nsurv,
                                                     int* __restrict__ next_nactive) {
  // The chunk's counts are staged in LDS by all four waves (coalesced), then wave 0 replays them: lane l
  // owns the contiguous segment [l seg, (l+1) seg).  Element h of lane l sits at h + l, which spreads
  // the lanes' same-offset reads over the banks.
  extern __shared__ int32_t lcnt[];
  const int p = blockIdx.x;
  if (err_by_h && threadIdx.x == 0) {   // what k_ransac_scan2 clears for the next round (the other parity's counters)
    next_nsurv[p] = 0;
    if (p == 0) *next_nactive = 0;
  }
  RansacProb pr = probs[p];
  if (pr.done) return;
  const int seg = (bcount + 63) / 64;
  {
    const int32_t* g = res_cnt + (int64_t)p * bmax;
    for (int h = threadIdx.x; h < bcount; h += 256) lcnt[h + h / seg] = g[h];
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const int32_t* cnt = lcnt + lane;  // cnt[h] for h in this lane's segment
  const int s0 = lane * seg, s1 = min(bcount, s0 + seg);
  // 1. exclusive prefix max of the counts over lanes, seeded with the carried best
  int lmax = 0;
  for (int h = s0; h < s1; ++h)
    if (it0 + h < pr.est_k) lmax = max(lmax, cnt[h]);
  int incl = lmax;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off);
    if (lane >= off) incl = max(incl, o);
  }
  int pre = __shfl_up(incl, 1);
  if (lane == 0) pre = 0;
  pre = max(pre, pr.best_cnt);
  // 2. first position where the loop of the reference would stop
  int stop = 0x7fffffff;
  {
    int cur = pre;
    int ek = cur > pr.best_cnt ? est_bound(cur, pr.m, ransac_n, log_1mc, pr.est_k) : pr.est_k;
    for (int h = s0; h < s1; ++h) {
      if (it0 + h >= ek) {
        stop = h;
        break;
      }
      const int c = cnt[h];
      if (c > cur) {
        cur = c;
        ek = est_bound(cur, pr.m, ransac_n, log_1mc, pr.est_k);
      }
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) stop = min(stop, __shfl_xor(stop, off));
  if (stop > bcount) stop = bcount;
  // 3. best count over the evaluated prefix, new bound
  int cmax = 0;
  for (int h = s0; h < min(s1, stop); ++h) cmax = max(cmax, cnt[h]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) cmax = max(cmax, __shfl_xor(cmax, off));
  int new_ek = pr.est_k;
  if (cmax > pr.best_cnt) new_ek = est_bound(cmax, pr.m, ransac_n, log_1mc, pr.est_k);
  // 4. candidates: evaluated hypotheses that tie for the best count (ascending order)
  int ncand = 0;
  // fused scan2: the sequential rule "take candidate c if the count rose or its error is strictly below the best so far" ends
  // at the FIRST candidate (ascending hypothesis) of the smallest error, provided the count rose or that error is below
  // the carried one -- a lexicographic (error, hypothesis) minimum over the lanes' segments
  unsigned long long e_min = ~0ULL;
  int h_min = 0x7fffffff;
  if (cmax > 0 && cmax >= pr.best_cnt) {
    if (err_by_h) {
      for (int h = s0; h < min(s1, stop); ++h)
        if (cnt[h] == cmax) {
          const unsigned long long e = err_by_h[(int64_t)p * bmax + h];
          if (e < e_min) {   // strict: the earlier hypothesis keeps a tie
            e_min = e;
            h_min = h;
          }
        }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long eo = __shfl_xor(e_min, off);
        const int ho = __shfl_xor(h_min, off);
        if (eo < e_min || (eo == e_min && ho < h_min)) {
          e_min = eo;
          h_min = ho;
        }
      }
    } else {
      int mine = 0;
      for (int h = s0; h < min(s1, stop); ++h) mine += cnt[h] == cmax;
      int incl2 = mine;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl2, off);
        if (lane >= off) incl2 += o;
      }
      int pos = incl2 - mine;
      ncand = __shfl(incl2, 63);
      for (int h = s0; h < min(s1, stop); ++h)
        if (cnt[h] == cmax) cand[(int64_t)p * bmax + pos++] = h;
    }
  }
  if (lane == 0) {
    const int consumed = it0 + stop;
    pr.est_k = new_ek;
    pr.n_cand = ncand;
    pr.chunk_max = cmax;
    if (consumed >= pr.est_k || consumed >= max_iter) {
      pr.done = 1;
      pr.iters = consumed < max_iter ? consumed : max_iter;
    } else {
      atomicAdd(n_active, 1);
    }
    if (err_by_h && h_min != 0x7fffffff && (cmax > pr.best_cnt || e_min < pr.best_err)) {
      pr.best_cnt = cmax;
      pr.best_err = e_min;
      pr.best_itr = it0 + h_min;
      for (int c = 0; c < 12; ++c) pr.best_T[c] = hyp[((int64_t)p * 12 + c) * bmax + h_min];
    }
    // (unfused: best_* are updated by scan2; keep everything else)
    probs[p] = pr;
  }
}

// cand_err is indexed by candidate slot (k_ransac_err) or, when by_h is set, by hypothesis
// (k_ransac_count_few computed the error of every survivor along with its count)
__global__ void k_ransac_scan2(RansacProb* probs, int n_prob, const double* __restrict__ hyp,
                               const int32_t* __restrict__ cand,
                               const unsigned long long* __restrict__ cand_err, int by_h, int it0,
                               int bmax, int32_t* __restrict__ next_nsurv, int* __restrict__ next_nactive) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  // last kernel of a round: clear the survivor / activity counters the NEXT round accumulates into (the other
  // parity's: this round's are still to be copied to the host) -- a hipMemsetAsync per round before
  next_nsurv[p] = 0;
  if (p == 0) *next_nactive = 0;
  RansacProb pr = probs[p];
  if (pr.n_cand <= 0) return;
  bool changed = false;
  int best_h = -1;
  for (int c = 0; c < pr.n_cand; ++c) {
    const unsigned long long e = cand_err[(int64_t)p * bmax + (by_h ? cand[(int64_t)p * bmax + c] : c)];
    if (pr.chunk_max > pr.best_cnt || e < pr.best_err) {
      pr.best_cnt = pr.chunk_max;
      pr.best_err = e;
      best_h = cand[(int64_t)p * bmax + c];
      changed = true;
    }
  }
  pr.n_cand = 0;
  if (changed) {
    pr.best_itr = it0 + best_h;
    for (int c = 0; c < 12; ++c) pr.best_T[c] = hyp[((int64_t)p * 12 + c) * bmax + best_h];
  }
  probs[p] = pr;
}

__global__ void k_ransac_finish(const RansacProb* __restrict__ probs, int n_prob, double scale,
                                float* __restrict__ T, int32_t* __restrict__ inliers,
                                double* __restrict__ rmse, int32_t* __restrict__ iters) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_prob) return;
  const RansacProb pr = probs[p];
  float* o = T + (int64_t)p * 16;
  if (pr.best_cnt > 0) {
    for (int c = 0; c < 12; ++c) o[c] = (float)pr.best_T[c];  // the reference's T_est.astype(np.float32)
  } else {
    for (int c = 0; c < 12; ++c) o[c] = (c % 5 == 0) ? 1.f : 0.f;
  }
  o[12] = 0.f;
  o[13] = 0.f;
  o[14] = 0.f;
  o[15] = 1.f;
  if (inliers) inliers[p] = pr.best_cnt;
  if (rmse)
    rmse[p] = pr.best_cnt > 0 ? sqrt(((double)pr.best_err / scale) / (double)pr.best_cnt) : 0.0;
  if (iters) iters[p] = pr.iters;
}

}  // namespace cs

using namespace cs;

namespace {
// prefilter diagnostics: {bound violations, hypotheses checked, sum of (bound - exact)} from
// CS_RANSAC_CHECK runs, {survivors, hypotheses evaluated} always
std::atomic<unsigned long long> g_pf_stats[5];  // zero-initialised (static storage)

// page-locked host staging buffer of the calling thread (grown on demand, freed at thread exit)
struct PinnedScratch {
  char* p = nullptr;
  size_t n = 0;
  ~PinnedScratch() {
    if (p) (void)hipHostFree(p);
  }
};
thread_local PinnedScratch t_pinned;
char* pinned_scratch(size_t bytes) {
  if (t_pinned.n < bytes) {
    if (t_pinned.p) (void)hipHostFree(t_pinned.p);
    t_pinned.p = nullptr;
    t_pinned.n = 0;
    void* q = nullptr;
    if (hipHostMalloc(&q, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    t_pinned.p = static_cast<char*>(q);
    t_pinned.n = bytes;
  }
  return t_pinned.p;
}

// The environment knobs of cs_ransac_batch.  All of them are read HERE, once per call: tests flip them between calls
// of one process, so none is cached.  INTEGRATION.md lists them.
struct Options {
  bool prefilter;          // CS_RANSAC_PREFILTER=0: exact-only RANSAC (the reference path of the identity tests)
  bool check;              // CS_RANSAC_CHECK=1: verify the bound against the exact count of EVERY hypothesis (slow; tests)
  int pf_nm;               // CS_RANSAC_PF_K=32: 2 = the two-MFMA form a_hi . (b_hi + b_lo); default 16: 1 = one MFMA,
                           // a_hi . b_hi' with the dropped term bounded per pair.  Same results (the exact kernels decide)
  bool stage2;             // CS_RANSAC_STAGE2=0: no K = 32 second stage on the survivors of the K = 16 form
  int first_chunk;         // CS_RANSAC_FIRST=<n>: iterations counted exactly before the prefilter starts (default 64)
  int force_jacobi;        // CS_RANSAC_JACOBI=1: every hypothesis through the Jacobi eigen-solver (the fallback of horn_qcp;
                           // the oracle's oc_rigid_fit_force_jacobi is its counterpart)
  bool overlap;            // CS_RANSAC_OVERLAP=0: every round on the caller's stream
  int trace_it0;           // CS_PF_TRACE=<it0>: per-workgroup trace of the prefilter launch of the round starting at it0
  const char* trace_file;  // (-1 = off), written to CS_PF_TRACE_FILE (tools/pf_trace.py)
};
Options read_options() {
  const char* pf = getenv("CS_RANSAC_PREFILTER");
  const char* ck = getenv("CS_RANSAC_CHECK");
  const char* k = getenv("CS_RANSAC_PF_K");
  const char* s2 = getenv("CS_RANSAC_STAGE2");
  const char* first = getenv("CS_RANSAC_FIRST");
  const char* jac = getenv("CS_RANSAC_JACOBI");
  const char* ov = getenv("CS_RANSAC_OVERLAP");
  const char* tr = getenv("CS_PF_TRACE");
  const char* trf = getenv("CS_PF_TRACE_FILE");
  Options o;
  o.prefilter = !(pf && pf[0] == '0');
  o.check = ck && ck[0] == '1';
  o.pf_nm = (k && atoi(k) == 32) ? 2 : 1;
  o.stage2 = !(s2 && s2[0] == '0');
  // The unfiltered chunk costs its hypotheses x ALL pairs in f64 (0.31 ms per 48-problem call at 256, twice per chair step);
  // with 64 the second chunk, [64, 512), is already prefiltered -- against the best of 64 hypotheses instead of 256, which
  // lets a few more of its hypotheses through to the exact kernels.  Results are the sequential loop's either way.
  // Clamped: a first chunk above BMAX would index the BMAX-sized scratch out of range, 0 would never advance the chunk loop.
  o.first_chunk = ((std::min(std::max(first ? atoi(first) : 64, 64), BMAX) + 63) / 64) * 64;
  o.force_jacobi = jac && atoi(jac) != 0;
  o.overlap = !(ov && ov[0] == '0');
  o.trace_it0 = tr ? atoi(tr) : -1;
  o.trace_file = trf ? trf : "/tmp/pf_trace.bin";
  return o;
}

// Every device buffer of a call, and the views of the buffers that exist once per round parity.
struct Scratch {
  int n_prob = 0;
  // per-round state in ONE block, so a round ends with one device->host copy (into pinned memory):
  // [RansacProb x n_prob | 2 x { n_surv int32 x n_prob (padded to 8 B) | n_active int32 (8 B) }]: the counters
  // exist once per round parity, the last scan kernel of a round clears the set of the next round
  size_t st_probs = 0, st_surv = 0, st_cnt = 0, st_bytes = 0;
  PoolBuf<char> state;
  char* h_state = nullptr;                 // the thread's pinned staging buffer (not owned)
  PoolBuf<float> pk;                       // SoA copy of the correspondences
  PoolBuf<float4> pair32;                  // 32-B rows for the sampling
  PoolBuf<double> hyp;                     // hypotheses (f64 R|t), one set per round parity
  PoolBuf<int32_t> res_cnt, cand;
  PoolBuf<unsigned long long> cand_err;
  // prefilter: f16 pair image (every problem padded to whole LDS stages), hypothesis rows, bounds, survivor lists
  PoolBuf<int64_t> off16;
  PoolBuf<_Float16> B16, A16;
  PoolBuf<float> c_h;
  PoolBuf<int32_t> cnt_up, hlist;
  PoolBuf<unsigned> pf_stat;
  PoolBuf<double> pf_sums;
  // second stage: K = 32 image, the compacted rows of the survivors, their bounds
  PoolBuf<_Float16> B32, A16s;
  PoolBuf<float> c_hs;
  PoolBuf<int32_t> cnt2;
  PoolBuf<int32_t> exact_dbg;              // CS_RANSAC_CHECK
  PoolBuf<unsigned long long> chk_stats;
  PoolBuf<int32_t> xcd_buf;                // placement tables, one per round parity (8 x n_prob entries each)
  PoolBuf<unsigned long long> trace;       // CS_PF_TRACE
  size_t trace_cap = 1;

  bool alloc(int n, int64_t tot1, int64_t rows16, int pf_nm, bool pf, bool stage2, bool check, bool tracing) {
    n_prob = n;
    st_probs = sizeof(RansacProb) * (size_t)n;
    st_surv = ((sizeof(int32_t) * (size_t)n + 7) / 8) * 8;
    st_cnt = st_surv + 8;
    st_bytes = st_probs + 2 * st_cnt;
    h_state = pinned_scratch(st_bytes);
    const size_t nb = (size_t)n * BMAX, ns2 = (size_t)n * PF_S2_CAP;
    if (tracing) trace_cap = (size_t)8 * n * 64 * 16 * 16;
    return h_state && state.alloc(st_bytes) && pk.alloc((size_t)tot1 * 6) && pair32.alloc((size_t)tot1 * 2) &&
           hyp.alloc(2 * nb * 12) && res_cnt.alloc(nb) && cand.alloc(nb) && cand_err.alloc(nb) && off16.alloc(n + 1) &&
           B16.alloc(pf ? (size_t)rows16 * pf_pitch(pf_nm) : 8) && A16.alloc(pf ? 2 * nb * PF_K : 8) &&
           c_h.alloc(pf ? 2 * nb : 1) && cnt_up.alloc(pf ? 2 * nb : 1) && hlist.alloc(pf ? nb : 1) &&
           pf_stat.alloc((size_t)n * PF_STAT) && pf_sums.alloc((size_t)n * 6) &&
           B32.alloc(stage2 ? (size_t)rows16 * PF_PITCH : 8) && A16s.alloc(stage2 ? ns2 * PF_K : 8) &&
           c_hs.alloc(stage2 ? ns2 : 1) && cnt2.alloc(stage2 ? ns2 : 1) &&
           exact_dbg.alloc(check ? nb : 1) && chk_stats.alloc(4) && xcd_buf.alloc((size_t)16 * n) && trace.alloc(trace_cap);
  }
  RansacProb* probs() const { return reinterpret_cast<RansacProb*>(state.p); }
  // counters of a round parity, device and host copy
  int32_t* nsurv(int par) const { return reinterpret_cast<int32_t*>(state.p + st_probs + par * st_cnt); }
  int* nactive(int par) const { return reinterpret_cast<int*>(state.p + st_probs + par * st_cnt + st_surv); }
  const int32_t* h_nsurv(int par) const { return reinterpret_cast<const int32_t*>(h_state + st_probs + par * st_cnt); }
  int h_nactive(int par) const { return *reinterpret_cast<const int*>(h_state + st_probs + par * st_cnt + st_surv); }
  // buffers of a round parity
  double* hyp_of(int par) const { return hyp.p + (size_t)par * n_prob * 12 * BMAX; }
  _Float16* A16_of(int par) const { return A16.p + (size_t)par * n_prob * BMAX * PF_K; }
  float* c_h_of(int par) const { return c_h.p + (size_t)par * n_prob * BMAX; }
  int32_t* cnt_up_of(int par) const { return cnt_up.p + (size_t)par * n_prob * BMAX; }
  int32_t* xcd_of(int par) const { return xcd_buf.p + (size_t)par * 8 * n_prob; }
};

struct Event {
  hipEvent_t e = nullptr;
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
};
// an error return must not hand the scratch buffers back to the pool while a side stream still uses
// them; on the normal path the final wait on the main stream is already ordered behind its events
struct SideDrain {
  hipStream_t st = nullptr;
  bool clean = false;
  ~SideDrain() {
    if (st && !clean) (void)hipStreamSynchronize(st);
  }
};

// One cs_ransac_batch call: arguments, options, scratch, streams and the state carried from round to round.
struct RansacCall {
  int n_prob = 0, ransac_n = 0, max_iter = 0, m_max = 0;
  uint64_t seed = 0;
  int64_t total = 0, tot1 = 1;
  double thr2 = 0.0, scale = 0.0, log_1mc = 0.0, tcap = 0.0;
  Options opt;
  bool pf_alloc = false, stage2 = false, check = false;   // what the options come to for THIS call
  std::vector<RansacProb> hp;                             // host copy of the per-problem state, as of the last read-back
  std::vector<int64_t> h_off16;
  std::vector<int32_t> h_xcd[2];
  Scratch sc;                                             // (declared before the drains: they are destroyed first)
  Event round_done, front_done[2], hyp_done[2];
  hipStream_t s = nullptr, side = nullptr, side_hyp = nullptr;
  SideDrain side_drain, side_hyp_drain;
  int max_surv_prev = 1 << 30;  // survivors per problem in the previous prefiltered round (unknown: many)
  unsigned long long tot_surv = 0, tot_eval = 0;
  size_t trace_n = 0;

  int init(const int64_t* h_off, int n, double max_corr, int rn, int iters, double confidence, uint64_t sd, hipStream_t st);
  int setup(const float* d_src, const float* d_tgt);
  int open_streams();
  RansacIn in() const { return RansacIn{sc.probs(), n_prob, m_max, tot1, sc.pk.p, sc.pair32.p}; }
  bool prefiltered(int it0) const { return pf_alloc && it0 >= opt.first_chunk; }
  // chunks: [0, first) counted exactly, [first, 512) in one piece, then doubling ([512, 1024), [1024, 2048), ...) up to BMAX
  int chunk_of(int it0) const {
    const int b = it0 < opt.first_chunk ? opt.first_chunk : it0 < 512 ? 512 - it0 : (it0 < BMAX ? it0 : BMAX);
    return b > max_iter - it0 ? max_iter - it0 : b;
  }
  // pair-range splits of the exact count of a whole chunk: enough workgroups for 256 CUs x several waves; the
  // correspondence range is split when the chunk is small (integer partial sums combine exactly)
  int chunk_splits(int tiles) const {
    int splits = (int)(4096 / ((int64_t)n_prob * tiles > 0 ? (int64_t)n_prob * tiles : 1));
    if (splits < 1) splits = 1;
    if (splits > 16) splits = 16;
    while (splits > 1 && m_max / splits < 4 * RC_CHUNK) --splits;
    return splits;
  }
  int place(int it0, int par, int* live);
  Front enqueue_front(int it0, int par, hipStream_t st);
  int back_half(const Front& cur);
  int count_chunk(const Front& cur, double eval_pairs);
  int count_survivors(const Front& cur, bool* err_known);
  bool read_back(const Front& cur);
  int finish(float* d_T, int32_t* d_inliers, double* d_rmse, int32_t* d_iters);
};

// Problem table, derived constants, options and scratch.
int RansacCall::init(const int64_t* h_off, int n, double max_corr, int rn, int iters, double confidence, uint64_t sd,
                     hipStream_t st) {
  n_prob = n;
  ransac_n = rn;
  max_iter = iters;
  seed = sd;
  s = st;
  total = h_off[n_prob] - h_off[0];
  tot1 = total ? total : 1;
  hp.resize(n_prob);
  h_off16.assign(n_prob + 1, 0);
  for (int p = 0; p < n_prob; ++p) {
    int64_t m = h_off[p + 1] - h_off[p];
    CS_REQUIRE(m >= 0 && m < (1LL << 24), CS_ERR_INVALID,
               "cs_ransac_batch: bad segment %d (a problem holds fewer than 2^24 correspondences)", p);
    RansacProb& pr = hp[p];
    memset(&pr, 0, sizeof(pr));
    pr.off = h_off[p];
    pr.m = (int32_t)m;
    pr.est_k = max_iter;
    pr.best_itr = -1;
    // Open3D returns the default (identity) result when there are fewer pairs than ransac_n
    pr.done = m < ransac_n ? 1 : 0;
    if (m > m_max) m_max = (int)m;
    h_off16[p + 1] = h_off16[p] + pf_padded(m);
  }
  // squared threshold (Open3D: max_correspondence_distance * max_correspondence_distance in double) and
  // the power-of-two fixed-point scale of the inlier error: terms d^2 * scale < 2^38, so the u64 sum over
  // a problem's (< 2^24) pairs cannot overflow and is exact in any order
  thr2 = max_corr * max_corr;
  int ex = 0;
  (void)frexp(thr2, &ex);
  scale = ldexp(1.0, 38 - ex);
  log_1mc = log(1.0 - confidence);  // -inf when confidence == 1: never exits early
  opt = read_options();
  // the prefilter needs pairs and at least one iteration behind the exactly counted first chunk
  pf_alloc = opt.prefilter && total > 0 && max_iter > opt.first_chunk;
  stage2 = pf_alloc && opt.pf_nm == 1 && opt.stage2;
  check = pf_alloc && opt.check;   // (no prefiltered round, nothing to check)
  tcap = opt.pf_nm == 2 ? 0.0 : PF_TCAP;
  const bool ok = sc.alloc(n_prob, tot1, h_off16[n_prob] ? h_off16[n_prob] : 1, opt.pf_nm, pf_alloc, stage2, check,
                           opt.trace_it0 >= 0);
  CS_REQUIRE(ok, CS_ERR_HIP, "cs_ransac_batch: scratch allocation failed");
  return CS_OK;
}

// Uploads the problem table and builds what every round reads: the packed pairs and, for the prefilter, the pair sums
// and the f16 images.
int RansacCall::setup(const float* d_src, const float* d_tgt) {
  // problems + zeroed counters in one upload (h_state is page-locked and not read before the first round ends)
  memset(sc.h_state, 0, sc.st_bytes);
  memcpy(sc.h_state, hp.data(), sc.st_probs);
  CS_HIP_CHECK(hipMemcpyAsync(sc.state.p, sc.h_state, sc.st_bytes, hipMemcpyHostToDevice, s));
  if (pf_alloc) {
    CS_HIP_CHECK(hipMemcpyAsync(sc.off16.p, h_off16.data(), sizeof(int64_t) * (n_prob + 1),
                                hipMemcpyHostToDevice, s));
    // the K = 32 image is the prefilter's own with CS_RANSAC_PF_K=32 (no K = 16 image then), the second stage's otherwise
    ransac_launch_images(in(), sc.off16.p, d_src, d_tgt, sc.pf_sums.p, sc.pf_stat.p, sc.chk_stats.p,
                         opt.pf_nm == 2 ? sc.B16.p : (stage2 ? sc.B32.p : nullptr), opt.pf_nm == 1 ? sc.B16.p : nullptr, tcap, s);
    CS_LAUNCH_CHECK();
  } else if (total > 0) {   // no prefilter in this call: the packed pairs alone
    ransac_launch_pack(in(), d_src, d_tgt, s);
    CS_LAUNCH_CHECK();
  }
  if (opt.trace_it0 >= 0) CS_HIP_CHECK(hipMemsetAsync(sc.trace.p, 0, sizeof(unsigned long long) * sc.trace_cap, s));
  return CS_OK;
}

// Events and the two side streams of the pipelined rounds (see cs_ransac_batch).
int RansacCall::open_streams() {
  for (Event* ev : {&round_done, &front_done[0], &front_done[1], &hyp_done[0], &hyp_done[1]})
    CS_HIP_CHECK(hipEventCreateWithFlags(&ev->e, hipEventDisableTiming));
  side = opt.overlap ? side_stream() : nullptr;
  // the hypotheses of a side-stream front half go to a THIRD stream: those of round i+2 are enqueued when round i
  // is known (their buffers, one set per parity, are free then) and run UNDER the prefilter of round i+1 instead of
  // behind it on the same stream (f64 vector work beside f16 matrix work)
  side_hyp = side ? side_stream(1) : nullptr;
  side_drain.st = side;
  side_hyp_drain.st = side_hyp;
  return CS_OK;
}

// Deals the problems that are live at iteration it0 to the 8 XCDs, longest first onto the least loaded XCD (host only).
// h_xcd[par] becomes the table [xcd][slot] -> problem (-1 = empty); returns the slots per XCD.
int RansacCall::place(int it0, int par, int* live) {
  std::vector<int> order;
  for (int p = 0; p < n_prob; ++p)
    if (!hp[p].done && hp[p].est_k > it0) order.push_back(p);
  *live = (int)order.size();
  std::sort(order.begin(), order.end(), [&](int a, int c) { return hp[a].m > hp[c].m; });
  std::vector<std::vector<int>> lists(8);
  int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int p : order) {
    int best = 0;
    for (int x = 1; x < 8; ++x)
      if (load[x] < load[best]) best = x;
    lists[best].push_back(p);
    load[best] += pf_padded(hp[p].m);
  }
  int pslots = 1;
  for (int x = 0; x < 8; ++x) pslots = std::max(pslots, (int)lists[x].size());
  std::vector<int32_t>& tab = h_xcd[par];
  tab.assign((size_t)8 * pslots, -1);
  for (int x = 0; x < 8; ++x)
    for (size_t i = 0; i < lists[x].size(); ++i) tab[(size_t)x * pslots + i] = lists[x][i];
  return pslots;
}

// Front half of the round that starts at it0: hypotheses (with their prefilter rows) and, from the second chunk on, the
// prefilter.  Independent of the carried best, so it may be enqueued on `st` = the side stream before the previous
// round is known; its skip tests read est_k / done while they may be updated (prob_view), and its placement is built
// from the state one round earlier: finished problems cost a few empty workgroups.
Front RansacCall::enqueue_front(int it0, int par, hipStream_t st) {
  Front f;
  f.it0 = it0;
  f.b = chunk_of(it0);
  f.par = par;
  f.pf = prefiltered(it0);
  f.on_side = st != s;
  const int b = f.b;
  int live = 0;
  f.pslots = place(it0, par, &live);
  const int pslots = f.pslots;
  // stream of the hypothesis kernel: the third stream for a prefiltered front half on the side stream
  hipStream_t sh = (f.on_side && f.pf && side_hyp) ? side_hyp : st;
  // the table travels as a kernel argument; rounds with more than XCD_SLOTS problems per XCD copy it to the device
  if (pslots <= XCD_SLOTS) {
    memcpy(f.xtab.v, h_xcd[par].data(), sizeof(int32_t) * 8 * pslots);
  } else {
    (void)hipMemcpyAsync(sc.xcd_of(par), h_xcd[par].data(), sizeof(int32_t) * 8 * pslots, hipMemcpyHostToDevice, sh);
    f.xcd_prob = sc.xcd_of(par);
  }
  _Float16* A16_r = f.pf ? sc.A16_of(par) : nullptr;
  float* c_h_r = f.pf ? sc.c_h_of(par) : nullptr;
  int32_t* cnt_up_r = f.pf ? sc.cnt_up_of(par) : nullptr;
  const int ptiles = (b + PF_HYP - 1) / PF_HYP;
  // 1024 workgroups are resident (4 per CU): split the pair range until there are >= 8 rounds of
  // workgroups, as long as a workgroup keeps >= 8 stages
  int psplits = (int)((8 * 1024 + (int64_t)live * ptiles - 1) / std::max<int64_t>((int64_t)live * ptiles, 1));
  if (psplits < 1) psplits = 1;
  if (psplits > 16) psplits = 16;
  while (psplits > 1 && m_max / psplits < 8 * PF_ROWS) --psplits;
  {
    ProfScope prof("ransac_hyp", sh);
    // the prefilter adds the partial counts of its pair-range splits with atomics: the hypothesis kernel clears them
    int32_t* fz = psplits > 1 ? cnt_up_r : nullptr;
    ransac_launch_hyp(in(), f, ransac_n, seed, opt.force_jacobi, sc.hyp_of(par), sc.pf_stat.p, sc.pf_sums.p, thr2, tcap, A16_r,
                      c_h_r, fz, sh);
  }
  if (f.pf) {
    if (sh != st) {   // the prefilter (side stream) follows the hypotheses (third stream)
      (void)hipEventRecord(hyp_done[par].e, sh);
      (void)hipStreamWaitEvent(st, hyp_done[par].e, 0);
    }
    ProfScope prof("ransac_pre", st);  // work units are added by the back half (state known there)
    unsigned long long* tr = (opt.trace_it0 == it0) ? sc.trace.p : nullptr;
    const unsigned nblk = ransac_launch_prefilter(opt.pf_nm, in(), sc.off16.p, sc.B16.p, A16_r, c_h_r, f, ptiles, psplits,
                                                  cnt_up_r, tr, nullptr, st);
    if (tr) trace_n = (size_t)nblk * 16;
  }
  if (f.on_side) (void)hipEventRecord(front_done[par].e, st);
  return f;
}

// Exact count of EVERY hypothesis of an unfiltered chunk (the first of a call, or all of them without the prefilter).
int RansacCall::count_chunk(const Front& cur, double eval_pairs) {
  const int b = cur.b;
  const int hpw = b <= 64 ? 64 : RC_HYP;      // hypotheses per workgroup
  const int tiles = (b + hpw - 1) / hpw;
  const int splits = chunk_splits(tiles);
  if (splits > 1 || hpw != RC_HYP)  // partial counts (pair-range splits, lane quarters) are combined with integer atomics
    CS_HIP_CHECK(hipMemset2DAsync(sc.res_cnt.p, sizeof(int32_t) * BMAX, 0, sizeof(int32_t) * b, n_prob, s));
  ProfScope prof("ransac_eval", s, 30.0 * eval_pairs);
  ransac_launch_count_chunk(in(), sc.hyp_of(cur.par), cur.it0, b, hpw, tiles, splits, thr2, sc.res_cnt.p, s);
  return CS_OK;
}

// Prefiltered round: the hypotheses whose bound reaches the carried best are listed, go through the K = 32 bound (second
// stage) and are counted exactly.  *err_known: their fixed-point errors are in cand_err (by hypothesis) as well.
int RansacCall::count_survivors(const Front& cur, bool* err_known) {
  const int b = cur.b;
  const double* hyp_r = sc.hyp_of(cur.par);
  const int32_t* cnt_up_r = sc.cnt_up_of(cur.par);
  int32_t* const d_nsurv = sc.nsurv(cur.par);   // cleared by the previous round's last scan kernel (or the upload)
  // This round's survivor counts are not known on the host: the previous round's pick the kernels (each is exact for
  // any count).  The first prefiltered round has no previous count, but a chunk of b <= FEW_MAX cannot leave more.
  const int surv_cap = std::min(max_surv_prev, b);
  const bool few = max_surv_prev <= FEW_MAX || b <= FEW_MAX;
  // the second stage runs when the few-survivor kernel will; its rows are written by the survivors kernel itself
  const bool run_s2 = stage2 && few && surv_cap <= PF_S2_CAP;
  Stage2Rows s2rows{};
  if (run_s2) {
    s2rows.A16 = sc.A16_of(cur.par);
    s2rows.c_h = sc.c_h_of(cur.par);
    s2rows.stat = sc.pf_stat.p;
    s2rows.tcap = tcap;
    s2rows.A16s = sc.A16s.p;
    s2rows.c_hs = sc.c_hs.p;
    s2rows.cnt2 = sc.cnt2.p;
  }
  ransac_launch_survivors(in(), cur, cnt_up_r, sc.res_cnt.p, sc.cand_err.p, sc.hlist.p, d_nsurv, s2rows, s);
  {
    ProfScope prof("ransac_eval", s);
    if (few) {
      if (run_s2) {
        // K = 32 bound of the survivors (rows compacted by k_ransac_survivors): one small prefilter launch over all pairs,
        // with the placement of the round's first stage.  Tiles for the WHOLE capacity: workgroups past a problem's list
        // leave at once.  k_ransac_count_few then skips the entries whose bound is below the best.
        const int s2tiles = std::max(1, (std::min(b, PF_S2_CAP) + PF_HYP - 1) / PF_HYP);
        int s2splits = 8;
        while (s2splits > 1 && m_max / s2splits < 8 * PF_ROWS) --s2splits;
        ransac_launch_prefilter(2, in(), sc.off16.p, sc.B32.p, sc.A16s.p, sc.c_hs.p, cur, s2tiles, s2splits, sc.cnt2.p, nullptr,
                                d_nsurv, s);
      }
      // survivor slots per (slice, problem): a workgroup loads its pairs once and walks its share of the survivors, so
      // FEW slots amortise the load (chair, same box: 2 / 4 / 8 / 16 slots -> 1 431 / 1 454 / 1 424 / 1 370 queries/s)
      const int fslots = surv_cap <= 256 ? 4 : 8;
      ransac_launch_count_few(in(), hyp_r, thr2, scale, sc.res_cnt.p, sc.cand_err.p, sc.hlist.p, d_nsurv, fslots,
                              run_s2 ? sc.cnt2.p : nullptr, s);
      *err_known = true;
    } else {
      ransac_launch_count_list(in(), hyp_r, cur.it0, b, thr2, sc.res_cnt.p, sc.hlist.p, d_nsurv, s);
    }
  }
  if (check) {   // both bounds against the exact count of every hypothesis of the chunk
    const int tiles = (b + RC_HYP - 1) / RC_HYP;
    const int splits = chunk_splits(tiles);
    CS_HIP_CHECK(hipMemset2DAsync(sc.exact_dbg.p, sizeof(int32_t) * BMAX, 0, sizeof(int32_t) * b, n_prob, s));
    ransac_launch_count_chunk(in(), hyp_r, cur.it0, b, RC_HYP, tiles, splits, thr2, sc.exact_dbg.p, s);
    ransac_launch_check(in(), cur, sc.exact_dbg.p, cnt_up_r, sc.hlist.p, d_nsurv, run_s2 ? sc.cnt2.p : nullptr, sc.chk_stats.p, s);
  }
  return CS_OK;
}

// Back half of a round, on the caller's stream: exact counts (of the whole chunk, or of the prefilter's survivors), then the
// replay of the chunk in iteration order -- the sequential RANSAC state (best, est_k, done) advances here.
int RansacCall::back_half(const Front& cur) {
  const int it0 = cur.it0, b = cur.b;
  // algorithmic work of this chunk (hp is the state before it): 30 FLOP per (evaluated hypothesis,
  // correspondence) (transform 18 + squared distance 8 + compare/accumulate) -- for the
  // exact count and for the prefilter alike (its matrix pipe executes 32 or 64 per pair: bench.py reports both)
  double eval_pairs = 0.0;
  for (int p = 0; p < n_prob; ++p) {
    if (hp[p].done) continue;
    const int nh = std::min(hp[p].est_k - it0, b);
    if (nh > 0) {
      eval_pairs += (double)nh * (double)hp[p].m;
      tot_eval += (unsigned long long)nh;
    }
  }
  bool err_known = false;  // the fixed-point errors of all candidates are already in cand_err (by hypothesis)
  if (!cur.pf) {
    if (int rc = count_chunk(cur, eval_pairs)) return rc;
  } else {
    prof_add_units("ransac_pre", 30.0 * eval_pairs);   // the units of the launch the front half bracketed
    if (int rc = count_survivors(cur, &err_known)) return rc;
  }
  static const hipError_t scan1_lds = hipFuncSetAttribute(
      reinterpret_cast<const void*>(k_ransac_scan1), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
  CS_REQUIRE(scan1_lds == hipSuccess, CS_ERR_HIP, "cs_ransac_batch: cannot reserve LDS for k_ransac_scan1");
  RansacProb* const d_probs = sc.probs();
  const double* hyp_r = sc.hyp_of(cur.par);
  int32_t* const next_nsurv = sc.nsurv(cur.par ^ 1);
  int* const next_nactive = sc.nactive(cur.par ^ 1);
  // scan1 replays the chunk and lists the candidates that tie for the best count.  When k_ransac_count_few has left the
  // error of every survivor it also picks the best of them; otherwise (unfiltered chunk, long survivor list) the errors
  // of the candidates are computed by k_ransac_err and k_ransac_scan2 picks.
  hipLaunchKernelGGL(k_ransac_scan1, dim3((unsigned)n_prob), dim3(256), sizeof(int32_t) * (b + 64), s, d_probs, n_prob,
                     sc.res_cnt.p, it0, b, BMAX, ransac_n, max_iter, log_1mc, sc.cand.p, sc.nactive(cur.par),
                     err_known ? sc.cand_err.p : (const unsigned long long*)nullptr, hyp_r, next_nsurv, next_nactive);
  if (!err_known) {
    ransac_launch_err(in(), hyp_r, sc.cand.p, thr2, scale, sc.cand_err.p, s);
    hipLaunchKernelGGL(k_ransac_scan2, dim3((unsigned)ceil_div(n_prob, 64)), dim3(64), 0, s,
                       d_probs, n_prob, hyp_r, sc.cand.p, sc.cand_err.p, 0, it0, BMAX, next_nsurv, next_nactive);
  }
  CS_LAUNCH_CHECK();
  return CS_OK;
}

// The round's state has arrived in h_state: survivor bookkeeping, then hp becomes the state after the round.
// Returns whether any problem is still active.
bool RansacCall::read_back(const Front& cur) {
  if (cur.pf) {   // (hp is still the state before the round: the problems that were live in it)
    const int32_t* h_surv = sc.h_nsurv(cur.par);
    max_surv_prev = 0;
    for (int p = 0; p < n_prob; ++p)
      if (!hp[p].done) {
        tot_surv += (unsigned long long)h_surv[p];
        if (h_surv[p] > max_surv_prev) max_surv_prev = h_surv[p];
      }
  }
  memcpy(hp.data(), sc.h_state, sc.st_probs);
  return sc.h_nactive(cur.par) != 0;
}

// Trace dump, statistics, results.
int RansacCall::finish(float* d_T, int32_t* d_inliers, double* d_rmse, int32_t* d_iters) {
  if (trace_n) {
    std::vector<unsigned long long> ht(trace_n);
    CS_HIP_CHECK(hipMemcpy(ht.data(), sc.trace.p, sizeof(unsigned long long) * trace_n, hipMemcpyDeviceToHost));
    FILE* f = fopen(opt.trace_file, "wb");
    if (f) {
      fwrite(ht.data(), sizeof(unsigned long long), trace_n, f);
      fclose(f);
    }
  }
  g_pf_stats[3] += tot_surv;
  g_pf_stats[4] += tot_eval;
  if (check) {
    unsigned long long h_stats[4] = {0, 0, 0, 0};
    CS_HIP_CHECK(hipMemcpyAsync(h_stats, sc.chk_stats.p, sizeof(h_stats), hipMemcpyDeviceToHost, s));
    CS_HIP_CHECK(hipStreamSynchronize(s));
    g_pf_stats[0] += h_stats[0];
    g_pf_stats[1] += h_stats[1];
    g_pf_stats[2] += h_stats[2];
    CS_REQUIRE(h_stats[0] == 0, CS_ERR_INTERNAL,
               "cs_ransac_batch: prefilter bound violated for %llu hypotheses", h_stats[0]);
  }
  hipLaunchKernelGGL(k_ransac_finish, dim3((unsigned)ceil_div(n_prob, 64)), dim3(64), 0, s,
                     sc.probs(), n_prob, scale, d_T, d_inliers, d_rmse, d_iters);
  CS_LAUNCH_CHECK();
  CS_HIP_CHECK(hipStreamSynchronize(s));
  side_drain.clean = true;
  side_hyp_drain.clean = true;
  return CS_OK;
}
}  // namespace

extern "C" {

void cs_ransac_prefilter_stats(uint64_t out[5], int reset) {
  for (int i = 0; i < 5; ++i) {
    if (out) out[i] = g_pf_stats[i].load();
    if (reset) g_pf_stats[i].store(0);
  }
}

int cs_ransac_batch(const float* d_src, const float* d_tgt, const int64_t* h_off, int n_prob,
                    double max_corr, int ransac_n, int max_iter, double confidence, uint64_t seed,
                    float* d_T, int32_t* d_inliers, double* d_rmse, int32_t* d_iters,
                    void* stream) {
  CS_REQUIRE(h_off && d_T, CS_ERR_INVALID, "cs_ransac_batch: NULL argument");
  CS_REQUIRE(ransac_n >= 3 && ransac_n <= 64, CS_ERR_INVALID,
             "cs_ransac_batch: ransac_n %d not in [3, 64]", ransac_n);
  CS_REQUIRE(max_corr > 0.0 && max_iter >= 1, CS_ERR_INVALID,
             "cs_ransac_batch: need max_corr > 0 and max_iter >= 1");
  CS_REQUIRE(confidence > 0.0 && confidence <= 1.0, CS_ERR_INVALID,
             "cs_ransac_batch: confidence must be in (0, 1]");
  if (n_prob <= 0) return CS_OK;
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const int64_t total = h_off[n_prob] - h_off[0];
  CS_REQUIRE(h_off[0] == 0 && total >= 0, CS_ERR_INVALID, "cs_ransac_batch: bad offsets");
  CS_REQUIRE(total == 0 || (d_src && d_tgt), CS_ERR_INVALID, "cs_ransac_batch: NULL correspondences");
  RansacCall c;
  if (int rc = c.init(h_off, n_prob, max_corr, ransac_n, max_iter, confidence, seed, s)) return rc;
  if (int rc = c.setup(d_src, d_tgt)) return rc;
  if (int rc = c.open_streams()) return rc;

  // A round = front half (hypotheses, f16 rows, prefilter: independent of the carried best) + back half (survivors,
  // exact counts, scans: the sequential RANSAC state), then ONE host wait for the round's state in pinned memory.
  // Streams: the back half always runs on the caller's stream s.  The front half of round i+1 is enqueued BEFORE the host
  // waits for round i: behind it on s while the rounds are short, on the low-priority c.side once rounds i and i+1 are both
  // prefiltered (its hypothesis kernel on c.side_hyp) -- so it fills the GPU while the back half of round i (many small
  // dependent kernels) and the host turnaround run.  s waits for a side-stream front half through front_done[parity].
  Front cur = c.enqueue_front(0, 0, s);
  CS_LAUNCH_CHECK();
  bool side_pending = false;  // the side stream holds work the main stream has not waited for
  int side_par = 0;
  while (true) {
    if (cur.on_side) {
      CS_HIP_CHECK(hipStreamWaitEvent(s, c.front_done[cur.par].e, 0));
      side_pending = false;
    }
    if (int rc = c.back_half(cur)) return rc;
    // the per-problem state (est_k, done), the survivor counts and the activity counter come back in
    // one copy behind a synchronisation the chunk loop needs anyway
    CS_HIP_CHECK(hipMemcpyAsync(c.sc.h_state, c.sc.state.p, c.sc.st_bytes, hipMemcpyDeviceToHost, s));
    CS_HIP_CHECK(hipEventRecord(c.round_done.e, s));
    Front nxt;
    const int it1 = cur.it0 + cur.b;
    const bool have_next = it1 < max_iter;
    if (have_next) {
      // on the side stream once both rounds are prefiltered: before that the rounds are short and the exact count of
      // round i+1 would compete with round i
      nxt = c.enqueue_front(it1, cur.par ^ 1, (c.side && cur.pf && c.prefiltered(it1)) ? c.side : s);
      if (nxt.on_side) {
        side_pending = true;
        side_par = nxt.par;
      }
      CS_LAUNCH_CHECK();
    }
    CS_HIP_CHECK(hipEventSynchronize(c.round_done.e));   // the host's only wait of a round
    const bool active = c.read_back(cur);
    if (!active || !have_next) break;
    cur = nxt;
  }
  // a speculative front half may still be running on the side stream (its workgroups see done = 1 and
  // leave): the scratch buffers go back to the main stream's pool only behind it
  if (side_pending) CS_HIP_CHECK(hipStreamWaitEvent(s, c.front_done[side_par].e, 0));
  return c.finish(d_T, d_inliers, d_rmse, d_iters);
}

}  // extern "C"
