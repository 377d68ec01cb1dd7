// Feature k-NN of the registration path, exact in f64 so that the returned indices equal those of the reference's
// SciPy routine:
//   cs_knn_feat <- KDTree(feat1).query(feat0, k)     (utils/find_nn.py:43-49, utils/eval_pose.py:48-79,
//                                                     utils/symmetry.py:145-179)
// The canonical distance is one f64 fma chain over the feature dimension in ascending order, sum_c (q_c - t_c)^2;
// ties go to the smaller row.  Every returned index / distance is that of the canonical chain.  There are two paths, and
// the fast one only decides WHICH rows get the canonical evaluation:
//   * default (16-d features, k <= 6; knn_f16.hip): k_knn_f16<1> bounds every query's k-th distance from tile minima,
//     k_knn_f16<0> shortlists by |t|^2 - 2 q.t on the f16 matrix cores, k_knn_rescore_f16 evaluates the shortlist with the
//     canonical chain, ranks it and VERIFIES it against the shortlist threshold; the queries that fail are recomputed by
//     k_knn_feat<16> (flagged tiles only).  CS_KNN_TWOPASS=0 drops the threshold pass; CS_KNN_STATS=1 counts the
//     recomputed queries (cs_knn_shortlist_stats; synchronises).
//   * CS_KNN_MFMA=0, and every other shape (3-d, 32-d, 33-d, k = 7 / 8; knn_exact.hip): k_knn_feat<DIM>, exhaustive on the
//     VALU -- the fallback of the f16 path and what the tests hold it against.
// Non-finite rows (include/corsair_hip.h): a candidate whose canonical distance is NaN or +inf is never a neighbour.  Every
// insertion test is a strict `<` against a list that starts at +inf, the tile minima are fminf / v_min3 (a NaN operand
// loses), and the budgets take their maxima with fmaxf (a NaN row does not enter seg_t2max; an infinite or huge one
// makes it +inf, which sends the whole segment to the exhaustive kernel).
// Labelled searches (part-to-part correspondences): the exhaustive kernel skips the rows of other labels; the f16 path
// visits the targets of a segment in label order and scans only the rows of the labels a workgroup wants.
// This unit: the driver (argument checks, work list, path choice), the C entries, and k_count_flags, which chamfer.hip
// reaches through count_flagged().
#include "knn.h"

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

static KnnOptions read_options() {
  KnnOptions o;
  o.path = env_first_is("CS_KNN_MFMA", '0') ? KnnOptions::EXHAUSTIVE : KnnOptions::F16;
  o.two_pass = !env_first_is("CS_KNN_TWOPASS", '0');
  o.stats = env_first_is("CS_KNN_STATS", '1');
  return o;
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
  CS_REQUIRE(dim == 16 || dim == 32 || dim == 33 || dim == 3, CS_ERR_UNSUPPORTED,
             "cs_knn_feat: feature dimension %d not supported (3, 16, 32, 33)", dim);
  CS_REQUIRE((d_qlabel == nullptr) == (d_tlabel == nullptr) &&
                 (d_qlabel == nullptr) == (d_perm == nullptr),
             CS_ERR_INVALID, "cs_knn_feat: labels and perm must be given together");
  if (n_prob <= 0) return CS_OK;
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  const KnnOptions opt = read_options();
  // the shortlist path takes 16-d features with k <= 6; everything else is the exhaustive kernel's
  const KnnOptions::Path path = (dim == 16 && k <= KNF_KK - 2) ? opt.path : KnnOptions::EXHAUSTIVE;
  const int qtile = 256;  // queries per workgroup of both paths
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
      w.pad = h_tseg[p];  // target segment (label-order tables of the shortlist path)
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
  if (path == KnnOptions::F16) {
    unsigned long long n_redone = 0;
    const int rc16 = knn_f16(call, opt, &n_redone);
    if (rc16 == CS_OK && opt.stats) {
      g_knn_stats[0] += (unsigned long long)out_row;
      g_knn_stats[1] += n_redone;
    }
    return rc16;
  }
  // CS_KNN_MFMA=0, and every shape the shortlist does not take (3-d, 32-d, 33-d, k > 6): the exhaustive VALU kernel
  ProfScope prof("knn", s, knn_flop);
  knn_exact_launch(call, nullptr, nullptr);
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // extern "C"
