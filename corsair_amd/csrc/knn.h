// What the k-NN units share: knn_exact.hip (the exhaustive kernel), knn_f16.hip (the f16 matrix-core shortlist path) and
// knn.hip (the driver and the C entries).  Every kernel is defined once, in one unit, and reached from the others through an
// ordinary host function that launches on the call's stream.
#pragma once
#include "nn_common.h"

namespace cs {

struct KnnWork {
  int64_t q0;   // first query row of the tile (row of d_qf)
  int64_t t0;   // first target row of the problem (row of d_tf)
  int64_t o0;   // first output row of the tile (problem-major)
  int32_t qn;   // query rows in this tile (<= 256)
  int32_t tn;   // target rows
  int32_t prob;
  int32_t pad;  // target segment (label-order tables and |t|^2 maxima of the f16 path)
};

constexpr int KNN_MAXK = 8;
constexpr int KNF_KK = 8;       // shortlist per lane of the f16 path (two lanes per query): it takes k <= KNF_KK - 2.  6 was
                                // measured: 23 of 189 517 queries fail the verification and their exhaustive recomputation
                                // costs more than the shorter lists save

// The environment switches of cs_knn_feat.
struct KnnOptions {
  enum Path { F16, EXHAUSTIVE };
  Path path;      // CS_KNN_MFMA: a value that begins with "0" exhaustive VALU kernel, anything else f16 matrix-core shortlist
  bool two_pass;  // CS_KNN_TWOPASS=0: the f16 shortlist pass alone, from +inf (no threshold pass)
  bool stats;     // CS_KNN_STATS=1: count the queries the f16 path recomputed exhaustively (synchronises)
};

// What cs_knn_feat has checked and built before it hands the call to one of the two paths.
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

// knn_exact.hip.  k_knn_feat<c.dim> over the work list.  tile_flag / qflag NULL: every tile, every query; otherwise only
// the flagged tiles run and only the flagged queries are written.  Launch only: the caller's CS_LAUNCH_CHECK covers it.
void knn_exact_launch(const KnnCall& c, const int32_t* tile_flag, const int32_t* qflag);

// knn_f16.hip.  16-d, k <= KNF_KK - 2: shortlist, canonical rescore and verification, exhaustive recomputation of the
// queries that fail it.  Under opt.stats *n_redone = the number of those queries (waits for the stream).
int knn_f16(const KnnCall& c, const KnnOptions& opt, unsigned long long* n_redone);

}  // namespace cs
