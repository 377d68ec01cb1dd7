// Partial views of point clouds: a virtual depth camera per segment.  Every row is splatted as a square of
// pixels into a z-buffer, and a row is visible when its own depth is within a tolerance of what the buffer holds at its
// centre pixel.  The specification is the comment of cs_render_views in include/corsair_hip.h; tests/view_ref.py restates
// it bit for bit.
//
// Four kernels per chunk of whole segments: k_view_fill (+inf into the buffer, zero into the stat rows), k_view_splat (one
// lane per row, one u64 atomicMin per covered pixel: positive finite doubles order as their bit patterns), k_view_resolve
// (one lane per row: the projection again, the same operations, then the comparison; three integer counts per wave) and
// k_view_export (one lane per pixel: the f32 image and the count of finite pixels).  Integer atomics only; no thread waits
// for another; every loop is bounded by the 33 x 33 pixels of the largest footprint.
#include <math.h>

#include <algorithm>
#include <vector>

#include "nn_common.h"
#include "view_plan.h"

namespace cs {
namespace {

static_assert(VIEW_OK == CS_OK && VIEW_INVALID == CS_ERR_INVALID && VIEW_UNSUPPORTED == CS_ERR_UNSUPPORTED,
              "view_plan.h restates the codes of corsair_hip.h");

constexpr int VW_BLOCK = 256;
constexpr unsigned long long VW_INF = 0x7ff0000000000000ull;   // the bits of +inf

struct ViewWork {
  int64_t seg0;   // first row of the segment (global)
  int32_t seg;    // the segment (global)
  int32_t r0;     // rows [r0, r1) of the segment, local
  int32_t r1;
};

struct ViewRow {
  double Z, u, v, h;
  int cu, cv;
  bool front, frame;
};

// floor(a) clamped as a double to [-1, hi], then converted: the conversion never leaves the range of an int
__device__ __forceinline__ int vw_edge(double a, double hi) {
  double f = floor(a);
  f = f < -1.0 ? -1.0 : f;
  f = f > hi ? hi : f;
  return (int)f;
}

// The header's "per row", operation by operation.  w, hgt = (double)width, (double)height; half_w = 0.5 * w,
// half_h = 0.5 * hgt and hf = (0.5 * focal) * point_size are formed once on the host (one IEEE operation each).
__device__ __forceinline__ ViewRow vw_row(const float* __restrict__ r, const double* __restrict__ cam, double w, double hgt,
                                          double half_w, double half_h, double focal, double hf) {
  const double x = (double)r[0], y = (double)r[1], z = (double)r[2];
  double P[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) P[c] = fma(cam[4 * c + 2], z, fma(cam[4 * c + 1], y, fma(cam[4 * c], x, cam[4 * c + 3])));
  ViewRow q = {};
  q.Z = P[2];
  q.front = fabs(P[0]) < INFINITY && fabs(P[1]) < INFINITY && fabs(P[2]) < INFINITY && P[2] > 0.0;   // false for NaN
  if (!q.front) return q;
  q.u = fma(focal, P[0] / q.Z, half_w);
  q.v = fma(focal, P[1] / q.Z, half_h);
  const double hh = hf / q.Z;
  q.h = hh < 16.0 ? hh : 16.0;
  const double fu = floor(q.u), fv = floor(q.v);
  q.frame = fu >= 0.0 && fu < w && fv >= 0.0 && fv < hgt;
  q.cu = q.frame ? (int)fu : 0;
  q.cv = q.frame ? (int)fv : 0;
  return q;
}

// One lane per pixel of the chunk: +inf; the first `segs` lanes also zero the chunk's stat rows.
__global__ __launch_bounds__(VW_BLOCK) void k_view_fill(unsigned long long* __restrict__ zbuf, int64_t pixels, int segs,
                                                        int32_t* __restrict__ stat) {
  const int64_t i = (int64_t)blockIdx.x * VW_BLOCK + threadIdx.x;
  if (i < pixels) zbuf[i] = VW_INF;
  if (i < segs) {
    int32_t* st = stat + 4 * i;
    st[0] = st[1] = st[2] = st[3] = 0;
  }
}

// One lane per row: the minimum of Z over the row's footprint.  precheck: the pixel is read first and skipped when it is
// already at least as near (the buffer only ever decreases, so a stale read can only cause an atomic that changes nothing).
__global__ __launch_bounds__(VW_BLOCK) void k_view_splat(const ViewWork* __restrict__ work, const float* __restrict__ xyz,
                                                         const double* __restrict__ cam, int seg_first, int width,
                                                         int height, double half_w, double half_h, double focal, double hf,
                                                         int precheck, unsigned long long* zbuf) {
  const ViewWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  if (row >= wk.r1) return;
  const double w = (double)width, hgt = (double)height;
  const ViewRow q = vw_row(xyz + (wk.seg0 + row) * 3, cam + 12 * (int64_t)wk.seg, w, hgt, half_w, half_h, focal, hf);
  if (!q.front) return;
  const int xa = max(vw_edge(q.u - q.h, w), 0), xb = min(vw_edge(q.u + q.h, w), width - 1);
  const int ya = max(vw_edge(q.v - q.h, hgt), 0), yb = min(vw_edge(q.v + q.h, hgt), height - 1);
  const unsigned long long bits = (unsigned long long)__double_as_longlong(q.Z);
  unsigned long long* zb = zbuf + (int64_t)(wk.seg - seg_first) * ((int64_t)height * width);
  for (int py = ya; py <= yb; ++py) {
    unsigned long long* line = zb + (int64_t)py * width;
    for (int px = xa; px <= xb; ++px) {
      if (precheck && line[px] <= bits) continue;
      atomicMin(line + px, bits);
    }
  }
}

// One lane per row: the mask and the three row counts (one integer atomicAdd per wave and count).
__global__ __launch_bounds__(VW_BLOCK) void k_view_resolve(const ViewWork* __restrict__ work, const float* __restrict__ xyz,
                                                           const double* __restrict__ cam, int seg_first, int width,
                                                           int height, double half_w, double half_h, double focal, double hf,
                                                           double depth_tol, const unsigned long long* __restrict__ zbuf,
                                                           uint8_t* __restrict__ visible, int32_t* __restrict__ stat) {
  const ViewWork wk = work[blockIdx.x];
  const int row = wk.r0 + threadIdx.x;
  bool front = false, frame = false, vis = false;
  if (row < wk.r1) {
    const ViewRow q = vw_row(xyz + (wk.seg0 + row) * 3, cam + 12 * (int64_t)wk.seg, (double)width, (double)height, half_w,
                             half_h, focal, hf);
    front = q.front;
    frame = q.front && q.frame;
    if (frame) {
      const int64_t at = (int64_t)(wk.seg - seg_first) * ((int64_t)height * width) + (int64_t)q.cv * width + q.cu;
      vis = q.Z - __longlong_as_double((long long)zbuf[at]) < depth_tol;
    }
    visible[wk.seg0 + row] = vis ? 1 : 0;
  }
  const int n_front = __popcll(__ballot(front)), n_frame = __popcll(__ballot(frame)), n_vis = __popcll(__ballot(vis));
  if ((threadIdx.x & 63) == 0) {
    int32_t* st = stat + 4 * (int64_t)wk.seg;
    if (n_front) atomicAdd(st + 0, n_front);
    if (n_frame) atomicAdd(st + 1, n_frame);
    if (n_vis) atomicAdd(st + 2, n_vis);
  }
}

// One lane per pixel; a workgroup stays inside one image (per_img workgroups per image).
__global__ __launch_bounds__(VW_BLOCK) void k_view_export(const unsigned long long* __restrict__ zbuf, int seg_first,
                                                          int64_t img, int per_img, float* __restrict__ depth,
                                                          int32_t* __restrict__ stat) {
  const int ls = blockIdx.x / per_img;
  const int64_t px = (int64_t)(blockIdx.x % per_img) * VW_BLOCK + threadIdx.x;
  bool finite = false;
  if (px < img) {
    const unsigned long long b = zbuf[(int64_t)ls * img + px];
    finite = b < VW_INF;
    if (depth) depth[(int64_t)(seg_first + ls) * img + px] = (float)__longlong_as_double((long long)b);
  }
  const int n = __popcll(__ballot(finite));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(stat + 4 * (int64_t)(seg_first + ls) + 3, n);
}

// the read before the atomic: CS_VIEW_PRECHECK (read per call), "0" turns it off.  The result does not depend on it.
bool view_precheck() {
  const char* e = getenv("CS_VIEW_PRECHECK");
  return !(e && e[0] == '0');
}

}  // namespace
}  // namespace cs

using namespace cs;

extern "C" {

int cs_render_views(const float* d_xyz, const int64_t* h_off, int n_seg, const double* d_cam, int width, int height,
                    double focal, double point_size, double depth_tol, uint8_t* d_visible, float* d_depth, int32_t* d_stat,
                    void* stream) {
  const char* who = "cs_render_views";
  char msg[192];
  const int bad = view_check_args(d_xyz, h_off, n_seg, d_cam, width, height, focal, point_size, depth_tol, d_visible, d_stat,
                                  msg, sizeof msg);
  CS_REQUIRE(bad == VIEW_OK, bad, "%s", msg);
  if (n_seg == 0) return CS_OK;
  const int64_t img = (int64_t)height * width;
  const std::vector<std::pair<int, int>> chunks = view_plan(n_seg, width, height, view_chunk_bytes());
  // the row blocks of the whole call, in the order of the segments; first_block[c] = the first one of chunk c
  std::vector<ViewWork> blocks;
  std::vector<size_t> first_block;
  int max_segs = 0;
  for (const auto& ch : chunks) {
    first_block.push_back(blocks.size());
    max_segs = std::max(max_segs, ch.second - ch.first);
    for (int sg = ch.first; sg < ch.second; ++sg) {
      const int64_t sn = h_off[sg + 1] - h_off[sg];
      for (int64_t r = 0; r < sn; r += VW_BLOCK)
        blocks.push_back(ViewWork{h_off[sg], (int32_t)sg, (int32_t)r, (int32_t)std::min(sn, r + VW_BLOCK)});
    }
  }
  first_block.push_back(blocks.size());
  const int per_img = (int)ceil_div(img, VW_BLOCK);
  CS_REQUIRE((int64_t)max_segs * per_img < (1LL << 31), CS_ERR_UNSUPPORTED,
             "%s: a chunk of %d images needs 2^31 workgroups or more (lower CS_VIEW_CHUNK_BYTES)", who, max_segs);
  hipStream_t s = (hipStream_t)stream;
  pool_use_stream(s);
  PoolBuf<ViewWork> d_blocks;
  PoolBuf<unsigned long long> zbuf((size_t)max_segs * (size_t)img);
  CS_REQUIRE(zbuf.p, CS_ERR_HIP, "%s: scratch allocation failed", who);
  if (!blocks.empty()) {
    const int rc = upload(d_blocks, blocks, s);
    if (rc) return rc;
  }
  const double half_w = 0.5 * (double)width, half_h = 0.5 * (double)height, hf = (0.5 * focal) * point_size;
  const int precheck = view_precheck() ? 1 : 0;
  ProfScope prof("view", s, (double)(h_off[n_seg] - h_off[0]));
  const dim3 block(VW_BLOCK);
  for (size_t c = 0; c < chunks.size(); ++c) {
    const int first = chunks[c].first, segs = chunks[c].second - chunks[c].first;
    const int64_t pixels = (int64_t)segs * img;
    const unsigned n_blocks = (unsigned)(first_block[c + 1] - first_block[c]);
    const ViewWork* work = d_blocks.p + first_block[c];
    hipLaunchKernelGGL(k_view_fill, dim3((unsigned)ceil_div(pixels, VW_BLOCK)), block, 0, s, zbuf.p, pixels, segs,
                       d_stat + 4 * (int64_t)first);
    if (n_blocks) {
      hipLaunchKernelGGL(k_view_splat, dim3(n_blocks), block, 0, s, work, d_xyz, d_cam, first, width, height, half_w, half_h,
                         focal, hf, precheck, zbuf.p);
      hipLaunchKernelGGL(k_view_resolve, dim3(n_blocks), block, 0, s, work, d_xyz, d_cam, first, width, height, half_w,
                         half_h, focal, hf, depth_tol, (const unsigned long long*)zbuf.p, d_visible, d_stat);
    }
    hipLaunchKernelGGL(k_view_export, dim3((unsigned)((int64_t)segs * per_img)), block, 0, s,
                       (const unsigned long long*)zbuf.p, first, img, per_img, d_depth, d_stat);
  }
  CS_LAUNCH_CHECK();
  return CS_OK;
}

}  // extern "C"
