// Resampling taps shared by the target model, the refiner glue and the refiner's backward kernels: one definition each, so that
// the fused kernels equal the unfused ones and the backward kernels are exact transposes of the forward ones.
#pragma once
#include "frtm_common.h"

// ATen bilinear source taps (upsample_bilinear2d, align_corners=False): src = max(scale * (d + .5) - .5, 0), i0 = (int)src,
// i1 = i0 + (i0 < n_in - 1), l1 = src - i0, l0 = 1 - l1.
__device__ __forceinline__ void bilinear_taps(int d, float scale, int n_in, int& i0, int& i1, float& l0, float& l1) {
  // (HIP's __fmul_rn / __fsub_rn are the plain operators: hipcc contracts the two into ONE fma, as it does in ATen's own device kernel,
  // so src is rounded once; tests/_native_refs.py: taps restates it that way and is held to torch's bilinear on the device)
  float src = __fsub_rn(__fmul_rn(scale, (float)d + 0.5f), 0.5f);
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  i1 = i0 + (i0 < n_in - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

// One bilinear sample of the (h,w) map p at pixel (y,x) of its (H,W) resize; the map itself when the sizes agree.
__device__ __forceinline__ float bilinear_at(const float* __restrict__ p, int h, int w, int H, int W, int y, int x) {
  if (h == H && w == W) return p[y * w + x];
  int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
  bilinear_taps(y, (float)h / (float)H, h, y0, y1, ly0, ly1);
  bilinear_taps(x, (float)w / (float)W, w, x0, x1, lx0, lx1);
  return ly0 * (lx0 * p[y0 * w + x0] + lx1 * p[y0 * w + x1]) + ly1 * (lx0 * p[y1 * w + x0] + lx1 * p[y1 * w + x1]);
}

// 2x polyphase bicubic taps (reference seg_network.py:75-126): the a = -0.75 cubic kernel at d = -0.25, i.e. cubic(1.25), cubic(.25),
// cubic(.75), cubic(1.75) = -27/256, 225/256, 67/256, -9/256.  Along one axis output 2a + 1 reads in[a-1 .. a+2] with (E0,E1,E2,E3)
// and output 2a reads in[a-2 .. a+1] with the reverse, indices clamped into the map (replicate border).
constexpr float PYR2X_E0 = -0.10546875f, PYR2X_E1 = 0.87890625f, PYR2X_E2 = 0.26171875f, PYR2X_E3 = -0.03515625f;
