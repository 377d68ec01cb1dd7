// The fused epilogue (BN affine / bias, residual add, ReLU) shared by the convolution fallbacks (conv.hip) and
// k_affine_act (rowops.hip).
#pragma once
#include "common.h"

namespace cs {

__device__ __forceinline__ float epilogue(float v, int c, const float* __restrict__ scale,
                                          const float* __restrict__ shift, const float* res_row,
                                          int relu) {
  if (scale)
    v = __fmaf_rn(v, scale[c], shift[c]);
  else if (shift)
    v = v + shift[c];
  if (res_row) v = v + res_row[c];
  if (relu) v = fmaxf(v, 0.0f);
  return v;
}

}  // namespace cs
