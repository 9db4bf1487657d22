// Fused glue kernels of the refinement network (reference model/seg_network.py:7-189).  The convolutions run on the MFMA
// conv kernels (conv_igemm.hip) with bias / BatchNorm / ReLU / residual folded into their epilogues; what is left between
// them -- bilinear / bicubic resampling, the score-channel injection of TSE, the channel-attention combine -- is HBM-bound
// element-wise work, one kernel each instead of 5-10 framework launches.
#include "frtm_common.h"
#include "resample_taps.h"
#include "per_frame.h"
#include "../../include/frtm_hip.h"

// out[pl] = bilinear(in[pl], (h,w) -> (H,W)) for `planes` maps.  One thread per output pixel computes the four taps once and
// walks all planes (coalesced along x in both tensors), instead of redoing the tap arithmetic per plane.
__global__ __launch_bounds__(256) void k_bilinear_resize(const float* __restrict__ in, int h, int w, float* __restrict__ out, int H, int W,
                                                          int planes, int planes_per_z) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= H * W) return;
  const int y = pix / W, x = pix - y * W;
  int y0, y1, x0, x1; float ly0, ly1, lx0, lx1;
  bilinear_taps(y, (float)h / (float)H, h, y0, y1, ly0, ly1);
  bilinear_taps(x, (float)w / (float)W, w, x0, x1, lx0, lx1);
  const float w00 = ly0 * lx0, w01 = ly0 * lx1, w10 = ly1 * lx0, w11 = ly1 * lx1;
  const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
  const int p0 = blockIdx.y * planes_per_z, p1 = min(planes, p0 + planes_per_z);
  const size_t hw = (size_t)h * w, HW = (size_t)H * W;
  for (int pl = p0; pl < p1; ++pl) {
    const float* p = in + pl * hw;
    out[pl * HW + pix] = w00 * p[o00] + w01 * p[o01] + w10 * p[o10] + w11 * p[o11];
  }
}

// The per-frame glue -- TSE score injection, CAB gate, CAB combine -- with the frame of sample s found as s / group: the bodies, their
// tiles and what they compute are in per_frame.h (the twins that read the frame from a table: ragged_group.hip).
__global__ __launch_bounds__(256) void k_tse_inject(const float* __restrict__ base, const float* __restrict__ bias, const float* __restrict__ ws,
                                                     const float* __restrict__ scores, int C, int h, int w, int H, int W,
                                                     float* __restrict__ out, int group) {
  tse_inject_body(base, bias, ws, scores, FrameByGroup{group}, C, h, w, H, W, out);
}

// deeper_group g > 0: samples s use deeper[s / g] (the pooled vector of the deepest level is shared by the objects of a frame);
// g = 0: one deeper map per sample.
__global__ __launch_bounds__(256) void k_cab_combine(const float* __restrict__ shallow, const float* __restrict__ gate, const float* __restrict__ deeper,
                                                      int C, int hd, int wd, int deeper_group, int H, int W, float* __restrict__ out) {
  cab_combine_body(shallow, gate, deeper, FrameByGroupOrOwn{deeper_group}, C, hd, wd, H, W, out);
}

// dp_group as deeper_group of k_cab_combine.
__global__ __launch_bounds__(256) void k_cab_gate(const float* __restrict__ sp, const float* __restrict__ dp, int dp_group,
                                                   const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
                                                   const float* __restrict__ b2, int oc, float* __restrict__ gate) {
  cab_gate_body(sp, dp, FrameByGroupOrOwn{dp_group}, W1, b1, W2, b2, oc, gate);
}

// 2x polyphase bicubic up-sampling, replicate border (seg_network.py:75-126): out = crop1(interleave(conv4x4(pad2(in)))).
// The taps are the a = -0.75 cubic kernel at d = -0.25 (even phase: PYR2X_E0 .. E3 of resample_taps.h) / d = -0.75 (odd phase: the reverse).
// One thread produces a COLUMN STRIP of PYR_Q vertically adjacent 2x2 output quads from the (PYR_Q + 4) x 5 input patch they share: 10 loads per
// quad instead of 25 and the index arithmetic once per strip (the quad-per-thread form was bound by its loads: 103 us for 64 planes x 10 samples
// of 120 x 214).  Same expressions per output as before (and as k_project_tail): results unchanged.
#define PYR_Q 4
__global__ __launch_bounds__(256) void k_pyrup2x(const float* __restrict__ in, int h, int w, float* __restrict__ out, size_t strips) {
  const float E[4] = {PYR2X_E0, PYR2X_E1, PYR2X_E2, PYR2X_E3};
  const int H = 2 * h, W = 2 * w;
  const int G = (h + PYR_Q - 1) / PYR_Q;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < strips; i += (size_t)gridDim.x * 256) {
    const int qx = (int)(i % w), qg = (int)((i / w) % G);
    const size_t pl = i / ((size_t)w * G);
    const int qy0 = qg * PYR_Q;
    const float* p = in + pl * (size_t)h * w;
    int cc[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) cc[c] = min(max(qx + c - 2, 0), w - 1);
    // horizontal pass of the strip's rows qy0-2 .. qy0+PYR_Q+1: column phase odd (taps reversed) uses cols 0..3, even phase uses cols 1..4
    float hx[PYR_Q + 4][2];
#pragma unroll
    for (int r = 0; r < PYR_Q + 4; ++r) {
      const float* pr = p + (size_t)min(max(qy0 + r - 2, 0), h - 1) * w;
      const float v0 = pr[cc[0]], v1 = pr[cc[1]], v2 = pr[cc[2]], v3 = pr[cc[3]], v4 = pr[cc[4]];
      hx[r][0] = E[3] * v0 + E[2] * v1 + E[1] * v2 + E[0] * v3;
      hx[r][1] = E[0] * v1 + E[1] * v2 + E[2] * v3 + E[3] * v4;
    }
    float* o = out + pl * (size_t)H * W + (size_t)(2 * qy0) * W + 2 * qx;
#pragma unroll
    for (int k = 0; k < PYR_Q; ++k) {
      if (qy0 + k >= h) break;
      // output rows 2qy (odd phase at input row qy) and 2qy+1 (even phase at input row qy+1): input rows qy-2 .. qy+2 = hx[k .. k+4]
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        o[(size_t)(2 * k) * W + c] = E[3] * hx[k][c] + E[2] * hx[k + 1][c] + E[1] * hx[k + 2][c] + E[0] * hx[k + 3][c];
        o[(size_t)(2 * k + 1) * W + c] = E[0] * hx[k + 1][c] + E[1] * hx[k + 2][c] + E[2] * hx[k + 3][c] + E[3] * hx[k + 4][c];
      }
    }
  }
}

// out[pl] = mean over the plane (adaptive_avg_pool2d to 1x1); one block per plane, dwordx4 loads, fixed summation order
__global__ __launch_bounds__(256) void k_plane_mean(const float* __restrict__ in, int HW, float* __restrict__ out) {
  __shared__ float red[16];
  const float* p = in + (size_t)blockIdx.x * HW;
  float acc = 0.f;
  if ((HW & 3) == 0 && ((size_t)p & 15) == 0) {
    const float4* p4 = (const float4*)p;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int i = threadIdx.x; i < HW / 4; i += 256) { const float4 v = p4[i]; a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w; }
    acc = (a0 + a1) + (a2 + a3);
  } else {
    for (int i = threadIdx.x; i < HW; i += 256) acc += p[i];
  }
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) out[blockIdx.x] = acc / (float)HW;
}


// ------------------------------------------------------------------------------------------
// Tail of the upsampler (seg_network.py:115-119): out = conv2(interpolate(up2(y), image_size)) for the single output channel,
// as ONE kernel.  Unfused, the 32-channel full-resolution tensor is written by the bicubic 2x, read and re-written by the
// bilinear resize and read again by the 3x3 conv (4 x 105 MB at 480p, 2 objects); here every workgroup rebuilds the patch
// of it that its 16x64 output tile needs in LDS, channel pair by channel pair, straight from y (26 MB):
//   A  y patch (replicate-clamped like PyrUpBicubic2d's padding)      -> ybuf
//   B  horizontal polyphase taps (even/odd output column)             -> hx
//   C  vertical polyphase taps                                        -> u    (the up2 output, rows/cols the tile needs)
//   D  ATen bilinear taps, zero outside the image (conv2 padding)     -> z
//   E  3x3 x 1-channel conv, 4 output rows per thread, accumulated over the channels in registers
// Same expressions as k_pyrup2x / k_bilinear_resize, so u and z are bit-identical to the unfused tensors.
// ------------------------------------------------------------------------------------------
#define PT_TH 16
#define PT_TW 64
#define PT_UR 22
#define PT_UC 76
#define PT_YR (PT_UR / 2 + 5)
#define PT_YC (PT_UC / 2 + 5)
#define PT_ZR (PT_TH + 2)
#define PT_ZC (PT_TW + 2)
#define PT_CG 2

__device__ __forceinline__ float pyr_taps(int odd, float a, float b, float c, float d) {
  const float E0 = PYR2X_E0, E1 = PYR2X_E1, E2 = PYR2X_E2, E3 = PYR2X_E3;
  return odd ? E0 * a + E1 * b + E2 * c + E3 * d : E3 * a + E2 * b + E1 * c + E0 * d;
}

// Every thread keeps the same elements of each stage for all channels, so all index / tap arithmetic happens once per tile
// (no per-element divisions inside the channel loop), and the y patch of the next channel pair is fetched into registers while
// the current pair goes through the stages.
__global__ __launch_bounds__(256, 4) void k_project_tail(const float* __restrict__ y, int C, int h, int w, const float* __restrict__ wgt,
                                                       const float* __restrict__ bias, float* __restrict__ out, int Ho, int Wo) {
  constexpr int NY = PT_YR * PT_YC, NYL = (PT_CG * NY + 255) / 256;          // y patch elements per thread
  constexpr int NZ = PT_ZR * PT_ZC, NZL = (NZ + 255) / 256;                  // z elements per thread (same for each channel)
  __shared__ float ybuf[PT_CG][PT_YR][PT_YC];
  __shared__ float ub[PT_CG][PT_UR][PT_UC];
  __shared__ float zb[PT_CG][PT_ZR][PT_ZC + 1];
  __shared__ int ri0[PT_ZR], ri1[PT_ZR], cj0[PT_ZC], cj1[PT_ZC];
  __shared__ float rl0[PT_ZR], rl1[PT_ZR], cl0[PT_ZC], cl1[PT_ZC];
  __shared__ int org[2];                                     // ur0, uc0
  const int tid = threadIdx.x, n = blockIdx.z;
  const int Y0 = blockIdx.y * PT_TH, X0 = blockIdx.x * PT_TW;
  const int Hu = 2 * h, Wu = 2 * w;
  // ---- tap tables of the z rows / columns this tile touches (-1: outside the image -> zero padding of conv2) ----
  if (tid < PT_ZR) {
    const int zy = Y0 - 1 + tid;
    int i0 = -1, i1 = -1; float l0 = 0.f, l1 = 0.f;
    if (zy >= 0 && zy < Ho) bilinear_taps(zy, (float)Hu / (float)Ho, Hu, i0, i1, l0, l1);
    ri0[tid] = i0; ri1[tid] = i1; rl0[tid] = l0; rl1[tid] = l1;
  }
  if (tid >= 64 && tid < 64 + PT_ZC) {
    const int j = tid - 64, zx = X0 - 1 + j;
    int i0 = -1, i1 = -1; float l0 = 0.f, l1 = 0.f;
    if (zx >= 0 && zx < Wo) bilinear_taps(zx, (float)Wu / (float)Wo, Wu, i0, i1, l0, l1);
    cj0[j] = i0; cj1[j] = i1; cl0[j] = l0; cl1[j] = l1;
  }
  __syncthreads();
  if (tid == 0) {
    int lo = 1 << 30;
    for (int i = 0; i < PT_ZR; ++i) if (ri0[i] >= 0) lo = min(lo, ri0[i]);
    org[0] = lo;
    lo = 1 << 30;
    for (int j = 0; j < PT_ZC; ++j) if (cj0[j] >= 0) lo = min(lo, cj0[j]);
    org[1] = lo;
  }
  __syncthreads();
  const int ur0 = org[0], uc0 = org[1];
  const int yr0 = (ur0 >> 1) - 2, yc0 = (uc0 >> 1) - 2;
  // ---- per-thread constants of each stage ----
  // A: element e = tid + k*256 of the [PT_CG][PT_YR][PT_YC] patch -> global offset inside one channel plane (replicate clamp)
  int a_goff[NYL], a_chan[NYL];
#pragma unroll
  for (int k = 0; k < NYL; ++k) {
    const int e = tid + k * 256;
    const int g = e / NY, r = (e - g * NY) / PT_YC, cc = e - g * NY - r * PT_YC;
    a_chan[k] = e < PT_CG * NY ? g : -1;
    a_goff[k] = min(max(yr0 + r, 0), h - 1) * w + min(max(yc0 + cc, 0), w - 1);
  }
  // BC: thread (g, j) builds column j of the up2 patch: 16 horizontal-tap values in registers, then the 22 vertical combinations
  const int bc_g = tid / PT_UC, bc_j = tid - bc_g * PT_UC;
  const bool bc_on = tid < PT_CG * PT_UC;
  const int bc_odd = (uc0 + bc_j) & 1, bc_b = ((uc0 + bc_j) >> 1) - 2 + bc_odd - yc0;
  const int par = ur0 & 1;
  // D: z elements e = tid + k*256 (same for each channel): LDS offsets into one channel's ub plane and the four weights
  int d_o00[NZL], d_o01[NZL], d_o10[NZL], d_o11[NZL], d_z[NZL];
  float d_w00[NZL], d_w01[NZL], d_w10[NZL], d_w11[NZL];
#pragma unroll
  for (int k = 0; k < NZL; ++k) {
    const int e = tid + k * 256;
    const int i = e / PT_ZC, j = e - i * PT_ZC;
    d_z[k] = e < NZ ? i * (PT_ZC + 1) + j : -1;
    const bool ok = e < NZ && ri0[e < NZ ? i : 0] >= 0 && cj0[j] >= 0;
    const int ii = e < NZ ? i : 0;
    const int a0 = ok ? ri0[ii] - ur0 : 0, a1 = ok ? ri1[ii] - ur0 : 0, b0 = ok ? cj0[j] - uc0 : 0, b1 = ok ? cj1[j] - uc0 : 0;
    d_o00[k] = a0 * PT_UC + b0; d_o01[k] = a0 * PT_UC + b1; d_o10[k] = a1 * PT_UC + b0; d_o11[k] = a1 * PT_UC + b1;
    d_w00[k] = ok ? rl0[ii] * cl0[j] : 0.f; d_w01[k] = ok ? rl0[ii] * cl1[j] : 0.f;
    d_w10[k] = ok ? rl1[ii] * cl0[j] : 0.f; d_w11[k] = ok ? rl1[ii] * cl1[j] : 0.f;
  }
  const int tx = tid & 63, ty = tid >> 6;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* yn = y + (size_t)n * C * h * w;
  const size_t hw = (size_t)h * w;
  float pre[NYL];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int k = 0; k < NYL; ++k) pre[k] = (a_chan[k] >= 0 && c0 + a_chan[k] < C) ? yn[(size_t)(c0 + a_chan[k]) * hw + a_goff[k]] : 0.f;
  };
  fetch(0);
  for (int c0 = 0; c0 < C; c0 += PT_CG) {
    const int ncg = min(PT_CG, C - c0);
    // A: registers -> ybuf, then start the next pair's loads
#pragma unroll
    for (int k = 0; k < NYL; ++k) if (a_chan[k] >= 0) (&ybuf[0][0][0])[tid + k * 256] = pre[k];
    __syncthreads();
    if (c0 + PT_CG < C) fetch(c0 + PT_CG);
    // BC: polyphase taps, horizontal then vertical (the order of k_pyrup2x)
    if (bc_on) {
      float hxv[PT_YR];
#pragma unroll
      for (int r = 0; r < PT_YR; ++r) {
        const float* v = &ybuf[bc_g][r][bc_b];
        hxv[r] = pyr_taps(bc_odd, v[0], v[1], v[2], v[3]);
      }
      // u row ur0 + i: odd = (i + par) & 1, first hx row = ((i + par) >> 1) + odd   (relative to yr0 = (ur0 >> 1) - 2)
      if (par == 0) {
#pragma unroll
        for (int i = 0; i < PT_UR; ++i) {
          const int odd = i & 1, bb = (i >> 1) + odd;
          ub[bc_g][i][bc_j] = pyr_taps(odd, hxv[bb], hxv[bb + 1], hxv[bb + 2], hxv[bb + 3]);
        }
      } else {
#pragma unroll
        for (int i = 0; i < PT_UR; ++i) {
          const int odd = (i + 1) & 1, bb = ((i + 1) >> 1) + odd;
          ub[bc_g][i][bc_j] = pyr_taps(odd, hxv[bb], hxv[bb + 1], hxv[bb + 2], hxv[bb + 3]);
        }
      }
    }
    __syncthreads();
    // D: bilinear taps (identity when the sizes agree: the second weights are exactly 0), zero outside the image
#pragma unroll
    for (int g = 0; g < PT_CG; ++g) {
      const float* up = &ub[g][0][0];
#pragma unroll
      for (int k = 0; k < NZL; ++k)
        if (d_z[k] >= 0)
          (&zb[g][0][0])[d_z[k]] = d_w00[k] * up[d_o00[k]] + d_w01[k] * up[d_o01[k]] + d_w10[k] * up[d_o10[k]] + d_w11[k] * up[d_o11[k]];
    }
    __syncthreads();
    // E: 3x3 conv, output rows ty*4 .. ty*4+3 at column tx
    for (int g = 0; g < ncg; ++g) {
      const float* f = wgt + (c0 + g) * 9;
      float zz[6][3];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int d = 0; d < 3; ++d) zz[r][d] = zb[g][ty * 4 + r][tx + d];
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[o] += zz[o + k / 3][k % 3] * f[k];
    }
    // next iteration: ybuf is rewritten after BC's barrier above; ub after the next A barrier; zb after two more barriers
  }
  const float b = bias ? bias[0] : 0.f;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int yy = Y0 + ty * 4 + o, xx = X0 + tx;
    if (yy < Ho && xx < Wo) out[((size_t)n * Ho + yy) * Wo + xx] = acc[o] + b;
  }
}

// ------------------------------------------------------------------------------------------
// Bicubic resampling of the Upsampler head (model/seg_network.py: Upsampler), F.interpolate(x, (H, W), mode='bicubic',
// align_corners=False) as documented:
//   scale = in / out per axis (a size is given, not a scale factor); source coordinate s = (dst + 0.5) * scale - 0.5, NOT clamped
//   at 0 for the cubic mode; four taps at floor(s) - 1 .. floor(s) + 2 with their indices clamped into the map; cubic convolution
//   with A = -0.75 at t = s - floor(s): weights k2(t + 1), k1(t), k1(1 - t), k2(2 - t) with
//   k1(x) = ((A + 2) x - (A + 3)) x^2 + 1   (|x| <= 1)  and  k2(x) = ((A x - 5A) x + 8A) x - 4A   (1 < |x| < 2).
// Both kernels below apply it separably, horizontal taps first, then vertical, with the same expressions: the fused tail's z patch
// equals the unfused resize up to the compiler's contraction choices.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int bc_taps(int d, float scale, float wt[4]) {
  const float A = -0.75f;
  const float s = __fsub_rn(__fmul_rn(scale, (float)d + 0.5f), 0.5f);
  const float f = floorf(s), t = s - f;
  const float x0 = t + 1.f, x3 = 2.f - t, x2 = 1.f - t;
  wt[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
  wt[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
  wt[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
  wt[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
  return (int)f - 1;                                         // first tap (unclamped)
}
__device__ __forceinline__ float bc_dot(const float wt[4], float a, float b, float c, float d) {
  return wt[0] * a + wt[1] * b + wt[2] * c + wt[3] * d;
}

// out[pl] = bicubic(in[pl], (h,w) -> (H,W)), any ratio up or down.  One thread per output pixel computes the taps once and walks
// `planes_per_z` planes (coalesced along x in the output), like k_bilinear_resize.  The unfused fallback of the Upsampler head.
__global__ __launch_bounds__(256) void k_bicubic_resize(const float* __restrict__ in, int h, int w, float* __restrict__ out, int H, int W,
                                                         int planes, int planes_per_z) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= H * W) return;
  const int y = pix / W, x = pix - y * W;
  float wy[4], wx[4];
  const int r0 = bc_taps(y, (float)h / (float)H, wy), c0 = bc_taps(x, (float)w / (float)W, wx);
  int ro[4], co[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    ro[k] = min(max(r0 + k, 0), h - 1) * w;
    co[k] = min(max(c0 + k, 0), w - 1);
  }
  const int p0 = blockIdx.y * planes_per_z, p1 = min(planes, p0 + planes_per_z);
  const size_t hw = (size_t)h * w, HW = (size_t)H * W;
  for (int pl = p0; pl < p1; ++pl) {
    const float* p = in + pl * hw;
    float hx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) hx[k] = bc_dot(wx, p[ro[k] + co[0]], p[ro[k] + co[1]], p[ro[k] + co[2]], p[ro[k] + co[3]]);
    out[pl * HW + pix] = bc_dot(wy, hx[0], hx[1], hx[2], hx[3]);
  }
}

// ------------------------------------------------------------------------------------------
// Tail of the Upsampler head: out = conv2(interpolate(y, (Ho, Wo), bicubic)) for the single output channel, as ONE kernel (the
// model is k_project_tail).  Every workgroup rebuilds in LDS the patch of the resized map that its 16x64 output tile and the conv
// halo read, BT_CG channels per round, straight from y; the full-resolution C-channel tensor never reaches HBM:
//   A  y patch (BT_YR x BT_YC source pixels, indices clamped into the map)      -> ybuf
//   B  horizontal cubic taps of the 66 z columns                                -> hb   (BT_YR x 66)
//   C  vertical cubic taps of the 18 z rows, zero outside the image (conv2 pad) -> zb   (18 x 66)
//   D  3x3 x 1-channel conv, 4 output rows per thread, accumulated over the channels in registers
// The source rows / columns a tile reads span floor(17 * scale) + 4 / floor(65 * scale) + 4 pixels, so the fixed patch bounds the
// ratio: upscale >= ~1.6x vertically and >= ~1.9x horizontally, any larger (480p / 720p / 1080p frames: ~4x from the 2x layer2 map).
// LDS 35 KB per workgroup: 4 workgroups (16 waves) per CU.
// ------------------------------------------------------------------------------------------
#define BT_TH 16
#define BT_TW 64
#define BT_ZR (BT_TH + 2)
#define BT_ZC (BT_TW + 2)
#define BT_YR 16
#define BT_YC 40
#define BT_CG 3
#define BT_BRG 3                                              // stage B: 3 row groups x 66 columns = 198 threads
#define BT_CCG 14                                             // stage C: 18 rows x 14 column groups = 252 threads

__global__ __launch_bounds__(256) void k_project_tail_bicubic(const float* __restrict__ y, int C, int h, int w, const float* __restrict__ wgt,
                                                               const float* __restrict__ bias, float* __restrict__ out, int Ho, int Wo) {
  constexpr int NY = BT_YR * BT_YC, NYL = (BT_CG * NY + 255) / 256;         // y patch elements per thread
  __shared__ float ybuf[BT_CG][BT_YR][BT_YC];
  __shared__ float hb[BT_CG][BT_YR][BT_ZC + 1];
  __shared__ float zb[BT_CG][BT_ZR][BT_ZC + 1];
  const int tid = threadIdx.x, n = blockIdx.z;
  const int Y0 = blockIdx.y * BT_TH, X0 = blockIdx.x * BT_TW;
  const float sy = (float)h / (float)Ho, sx = (float)w / (float)Wo;
  float wt[4];
  // patch origin = first tap of the first z row / column inside the image (the taps only grow along the tile)
  const int yr0 = bc_taps(max(Y0 - 1, 0), sy, wt), yc0 = bc_taps(max(X0 - 1, 0), sx, wt);
  // A: element e = tid + k*256 of the [BT_CG][BT_YR][BT_YC] patch -> offset inside one channel plane, -1 past the patch
  int a_goff[NYL], a_chan[NYL];
#pragma unroll
  for (int k = 0; k < NYL; ++k) {
    const int e = tid + k * 256;
    const int g = e / NY, r = (e - g * NY) / BT_YC, cc = e - g * NY - r * BT_YC;
    a_chan[k] = e < BT_CG * NY ? g : -1;
    a_goff[k] = min(max(yr0 + r, 0), h - 1) * w + min(max(yc0 + cc, 0), w - 1);
  }
  // B: thread (b_rg, b_j) forms z column b_j of the patch rows b_rg, b_rg + 3, ...: that column's taps stay in registers
  const int b_rg = tid / BT_ZC, b_j = tid - b_rg * BT_ZC;
  const bool b_on = tid < BT_BRG * BT_ZC;
  float b_w[4];
  const int zx = X0 - 1 + b_j;
  const int b_c = min(max(bc_taps(min(max(zx, 0), Wo - 1), sx, b_w) - yc0, 0), BT_YC - 4);
  // C: thread (c_i, c_jg) forms z row c_i at the columns c_jg, c_jg + 14, ...; rows / columns outside the image are conv2's zeros
  const int c_i = min(tid / BT_CCG, BT_ZR - 1), c_jg = tid - (tid / BT_CCG) * BT_CCG;
  const bool c_on = tid < BT_ZR * BT_CCG;
  const int zy = Y0 - 1 + c_i;
  float c_w[4];
  const int c_r = min(max(bc_taps(min(max(zy, 0), Ho - 1), sy, c_w) - yr0, 0), BT_YR - 4);
  const bool c_row = zy >= 0 && zy < Ho;
  const int tx = tid & 63, ty = tid >> 6;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const float* yn = y + (size_t)n * C * h * w;
  const size_t hw = (size_t)h * w;
  float pre[NYL];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int k = 0; k < NYL; ++k) pre[k] = (a_chan[k] >= 0 && c0 + a_chan[k] < C) ? yn[(size_t)(c0 + a_chan[k]) * hw + a_goff[k]] : 0.f;
  };
  fetch(0);
  for (int c0 = 0; c0 < C; c0 += BT_CG) {
    const int ncg = min(BT_CG, C - c0);
    // A: registers -> ybuf, then start the next group's loads
#pragma unroll
    for (int k = 0; k < NYL; ++k) if (a_chan[k] >= 0) (&ybuf[0][0][0])[tid + k * 256] = pre[k];
    __syncthreads();
    if (c0 + BT_CG < C) fetch(c0 + BT_CG);
    // B: horizontal taps
    if (b_on) {
#pragma unroll
      for (int g = 0; g < BT_CG; ++g)
#pragma unroll
        for (int m = 0; m < (BT_YR + BT_BRG - 1) / BT_BRG; ++m) {
          const int r = b_rg + BT_BRG * m;
          if (r < BT_YR) {
            const float* v = &ybuf[g][r][b_c];
            hb[g][r][b_j] = bc_dot(b_w, v[0], v[1], v[2], v[3]);
          }
        }
    }
    __syncthreads();
    // C: vertical taps
    if (c_on) {
#pragma unroll
      for (int g = 0; g < BT_CG; ++g)
#pragma unroll
        for (int m = 0; m < (BT_ZC + BT_CCG - 1) / BT_CCG; ++m) {
          const int j = c_jg + BT_CCG * m;
          if (j < BT_ZC) {
            const bool in = c_row && X0 - 1 + j >= 0 && X0 - 1 + j < Wo;
            zb[g][c_i][j] = in ? bc_dot(c_w, hb[g][c_r][j], hb[g][c_r + 1][j], hb[g][c_r + 2][j], hb[g][c_r + 3][j]) : 0.f;
          }
        }
    }
    __syncthreads();
    // D: 3x3 conv, output rows ty*4 .. ty*4+3 at column tx
    for (int g = 0; g < ncg; ++g) {
      const float* f = wgt + (c0 + g) * 9;
      float zz[6][3];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int d = 0; d < 3; ++d) zz[r][d] = zb[g][ty * 4 + r][tx + d];
#pragma unroll
      for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[o] += zz[o + k / 3][k % 3] * f[k];
    }
    // next round: ybuf is rewritten after B's barrier above; hb after the next A barrier; zb after two more barriers
  }
  const float b = bias ? bias[0] : 0.f;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int yy = Y0 + ty * 4 + o, xx = X0 + tx;
    if (yy < Ho && xx < Wo) out[((size_t)n * Ho + yy) * Wo + xx] = acc[o] + b;
  }
}

// ------------------------------------------------------------------------------------------
// conv2 (3x3, C -> 1) after two resampling steps is linear in y, and the channel sum commutes with the resampling:
//   conv2(R(U(y)))(p) = sum_t sum_c w[c][t] R(U(y_c))(p + t) = sum_t R(U(Y_t))(p + t),     Y_t = sum_c w[c][t] y_c   (t = one of the nine taps)
// so the tail only has to resample NINE maps instead of C = 32 (round 5; k_project_tail then runs on Y with one-hot weights).  This kernel forms
// Y (n,9,h,w) from y (n,C,h,w): one pass over y, V pixels per thread, the nine weights of a channel wave-uniform (scalar loads).
// ------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void k_tap_mix(const float* __restrict__ y, const float* __restrict__ w, int C, int hwv, float* __restrict__ out) {
  typedef float fv __attribute__((ext_vector_type(V)));
  const int i = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (i >= hwv) return;
  fv acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = fv(0.f);
  const fv* yp = (const fv*)(y + (size_t)n * C * hwv * V) + i;
  int c = 0;
  for (; c + 4 <= C; c += 4) {                              // four channels' loads in flight
    fv v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = yp[(size_t)(c + u) * hwv];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[t] += w[(c + u) * 9 + t] * v[u];
  }
  for (; c < C; ++c) {
    const fv v = yp[(size_t)c * hwv];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] += w[c * 9 + t] * v;
  }
  fv* op = (fv*)(out + (size_t)n * 9 * hwv * V) + i;
#pragma unroll
  for (int t = 0; t < 9; ++t) op[(size_t)t * hwv] = acc[t];
}

extern "C" {

int frtm_tap_mix(const float* y, int n, int C, int hw, const float* w3x3, float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(y && w3x3 && out && n > 0 && C > 0 && hw > 0, "frtm_tap_mix: bad argument");
  FRTM_CHECK_ARG(n <= 65535, "frtm_tap_mix: at most 65535 samples per call (got %d)", n);
  if (hw % 4 == 0 && ((size_t)y % 16 == 0) && ((size_t)out % 16 == 0))
    k_tap_mix<4><<<dim3(ceil_div(hw / 4, 256), n), 256, 0, (hipStream_t)stream>>>(y, w3x3, C, hw / 4, out);
  else
    k_tap_mix<1><<<dim3(ceil_div(hw, 256), n), 256, 0, (hipStream_t)stream>>>(y, w3x3, C, hw, out);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_bilinear_resize(const float* in, int planes, int h, int w, float* out, int H, int W, frtm_stream_t stream) {
  FRTM_CHECK_ARG(in && out && planes > 0 && h > 0 && w > 0 && H > 0 && W > 0, "frtm_bilinear_resize: bad argument");
  FRTM_CHECK_ARG((size_t)H * W < 0x7fffffff && (size_t)h * w < 0x7fffffff, "frtm_bilinear_resize: map too large");
  const int ppz = 8;
  FRTM_CHECK_ARG(ceil_div(planes, ppz) <= 65535, "frtm_bilinear_resize: at most %d planes per call (got %d)", 65535 * ppz, planes);
  dim3 g(ceil_div(H * W, 256), ceil_div(planes, ppz));
  k_bilinear_resize<<<g, 256, 0, (hipStream_t)stream>>>(in, h, w, out, H, W, planes, ppz);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_tse_inject(const float* base, const float* bias, const float* ws, const float* scores, int n, int group, int C, int h, int w, int H,
                    int W, float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(base && bias && ws && scores && out && n > 0 && C > 0 && group > 0 && n % group == 0, "frtm_tse_inject: bad argument");
  FRTM_CHECK_ARG(h > 0 && w > 0 && H > 0 && W > 0, "frtm_tse_inject: map sizes must be positive (scores %d x %d, maps %d x %d)", h, w, H, W);
  FRTM_CHECK_ARG((size_t)H * W < 0x7fffffff && (size_t)h * w < 0x7fffffff, "frtm_tse_inject: map too large");
  FRTM_CHECK_ARG((size_t)n * INJ_CG <= 65535, "frtm_tse_inject: at most %d samples per call (got %d)", 65535 / INJ_CG, n);
  FRTM_CHECK_ARG(ceil_div(H, INJ_TH) <= 65535, "frtm_tse_inject: at most %d rows per map (got %d)", 65535 * INJ_TH, H);
  dim3 g(ceil_div(W, INJ_TW), ceil_div(H, INJ_TH), n * INJ_CG);
  k_tse_inject<<<g, 256, 0, (hipStream_t)stream>>>(base, bias, ws, scores, C, h, w, H, W, out, group);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_cab_combine(const float* shallow, const float* gate, const float* deeper, int n, int C, int hd, int wd, int deeper_group, int H,
                     int W, float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(shallow && gate && deeper && out && n > 0 && C > 0 && deeper_group >= 0, "frtm_cab_combine: bad argument");
  FRTM_CHECK_ARG(hd > 0 && wd > 0 && H > 0 && W > 0, "frtm_cab_combine: map sizes must be positive (deeper %d x %d, maps %d x %d)", hd, wd, H, W);
  FRTM_CHECK_ARG(deeper_group == 0 || n % deeper_group == 0, "frtm_cab_combine: %d samples are not a multiple of deeper_group %d", n, deeper_group);
  FRTM_CHECK_ARG((size_t)n * C <= 65535 && (size_t)H * W < 0x7fffffff, "frtm_cab_combine: at most 65535 planes per call");
  dim3 g(ceil_div(H, CAB_RB), n * C);
  k_cab_combine<<<g, 256, 0, (hipStream_t)stream>>>(shallow, gate, deeper, C, hd, wd, deeper_group, H, W, out);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_cab_gate(const float* sp, const float* dp, int dp_group, const float* W1, const float* b1, const float* W2, const float* b2,
                  int n, int oc, float* gate, frtm_stream_t stream) {
  FRTM_CHECK_ARG(sp && dp && W1 && b1 && W2 && b2 && gate && n > 0 && oc > 0, "frtm_cab_gate: bad argument");
  FRTM_CHECK_ARG(dp_group >= 0, "frtm_cab_gate: dp_group must not be negative (got %d)", dp_group);
  // 7 oc floats of dynamic LDS; 64 KB is what a launch gets without raising the kernel's limit
  FRTM_CHECK_ARG((size_t)7 * oc * sizeof(float) <= 65536, "frtm_cab_gate: oc = %d needs %zu bytes of LDS, more than the 65536 of a default launch",
                 oc, (size_t)7 * oc * sizeof(float));
  FRTM_CHECK_ARG(dp_group == 0 || n % dp_group == 0, "frtm_cab_gate: %d samples are not a multiple of dp_group %d", n, dp_group);
  FRTM_CHECK_ARG(oc % 4 == 0, "frtm_cab_gate: oc must be a multiple of 4 (got %d)", oc);
  k_cab_gate<<<n, 256, 7 * oc * sizeof(float), (hipStream_t)stream>>>(sp, dp, dp_group, W1, b1, W2, b2, oc, gate);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_pyrup2x(const float* in, int planes, int h, int w, float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(in && out && planes > 0 && h > 0 && w > 0, "frtm_pyrup2x: bad argument");
  const size_t strips = (size_t)planes * ((h + PYR_Q - 1) / PYR_Q) * w;
  k_pyrup2x<<<(int)min((strips + 255) / 256, (size_t)16384), 256, 0, (hipStream_t)stream>>>(in, h, w, out, strips);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

// Whether the fused tail takes a (h,w) -> (Ho,Wo) resize of the map handed to it: the LDS patch of a 16x64 output tile (+1 conv halo) bounds
// the ratio.  Host only; the one definition of the rule (the argument checks below, ops.project_tail_fits).
int frtm_project_tail_fits(int bicubic, int h, int w, int Ho, int Wo) {
  if (h <= 0 || w <= 0 || Ho <= 0 || Wo <= 0) return 0;
  if (bicubic) {
    // the source rows / columns an 18 x 66 z patch reads through the cubic taps (one row / column of margin for the rounding of the
    // source coordinates)
    const double sy = (double)h / Ho, sx = (double)w / Wo;
    return (int)((BT_ZR - 1) * sy) + 6 <= BT_YR && (int)((BT_ZC - 1) * sx) + 6 <= BT_YC;
  }
  // the rows / columns of the 2x-upsampled map that the patch reads through the bilinear taps
  const double sy = 2.0 * h / Ho, sx = 2.0 * w / Wo;
  return (int)(PT_ZR * sy) + 3 <= PT_UR && (int)(PT_ZC * sx) + 3 <= PT_UC;
}

int frtm_project_tail(const float* y, int n, int C, int h, int w, const float* w3x3, const float* bias, int Ho, int Wo, float* out,
                      frtm_stream_t stream) {
  FRTM_CHECK_ARG(y && w3x3 && out && n > 0 && C > 0 && h > 1 && w > 1 && Ho > 0 && Wo > 0, "frtm_project_tail: bad argument");
  FRTM_CHECK_ARG(n <= 65535, "frtm_project_tail: at most 65535 samples per call (got %d)", n);
  FRTM_CHECK_ARG(frtm_project_tail_fits(0, h, w, Ho, Wo),
                 "frtm_project_tail: resize ratio %.3f x %.3f outside the fused kernel's patch (use pyrup2x + bilinear_resize + filter_scores)",
                 2.0 * h / Ho, 2.0 * w / Wo);
  dim3 g(ceil_div(Wo, PT_TW), ceil_div(Ho, PT_TH), n);
  k_project_tail<<<g, 256, 0, (hipStream_t)stream>>>(y, C, h, w, w3x3, bias, out, Ho, Wo);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_bicubic_resize(const float* in, int planes, int h, int w, float* out, int H, int W, frtm_stream_t stream) {
  FRTM_CHECK_ARG(in && out && planes > 0 && h > 0 && w > 0 && H > 0 && W > 0, "frtm_bicubic_resize: bad argument");
  FRTM_CHECK_ARG((size_t)H * W < 0x7fffffff && (size_t)h * w < 0x7fffffff, "frtm_bicubic_resize: map too large");
  const int ppz = 8;
  dim3 g(ceil_div(H * W, 256), ceil_div(planes, ppz));
  k_bicubic_resize<<<g, 256, 0, (hipStream_t)stream>>>(in, h, w, out, H, W, planes, ppz);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_project_tail_bicubic(const float* y, int n, int C, int h, int w, const float* w3x3, const float* bias, int Ho, int Wo, float* out,
                              frtm_stream_t stream) {
  FRTM_CHECK_ARG(y && w3x3 && out && n > 0 && C > 0 && h > 0 && w > 0 && Ho > 0 && Wo > 0, "frtm_project_tail_bicubic: bad argument");
  FRTM_CHECK_ARG(frtm_project_tail_fits(1, h, w, Ho, Wo),
                 "frtm_project_tail_bicubic: resize ratio %.3f x %.3f outside the fused kernel's patch (use bicubic_resize + filter_scores)",
                 (double)h / Ho, (double)w / Wo);
  dim3 g(ceil_div(Wo, BT_TW), ceil_div(Ho, BT_TH), n);
  FRTM_CHECK_ARG(n <= 65535, "frtm_project_tail_bicubic: at most 65535 samples per call");
  k_project_tail_bicubic<<<g, 256, 0, (hipStream_t)stream>>>(y, C, h, w, w3x3, bias, out, Ho, Wo);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_plane_mean(const float* in, int planes, int HW, float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(in && out && planes > 0 && HW > 0, "frtm_plane_mean: bad argument");
  k_plane_mean<<<planes, 256, 0, (hipStream_t)stream>>>(in, HW, out);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

}  // extern "C"
