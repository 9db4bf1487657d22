// Format-aware forms of the three bf16x1 conv kernels (opt-in bf16x1_act trunk mode): the 1x1 stride-1 kernel of conv_bf16x1.hip (layout 6), the 3x3
// pad-1 stride-1 kernel of conv3x3_bf16x1.hip (7) and the 3x3 pad-1 stride-2 kernel of conv3x3s2_bf16x1.hip (8), each with its activation input,
// its residual and its output independently in fp32 NCHW (FRTM_ACT_FP32) or in the channel-blocked bf16 layout FRTM_ACT_BF16 of include/frtm_hip.h:
//
//   element (img, c, p) of a (B, C, H, W) tensor at bf16 index ((img * C/8 + c/8) * H*W + p) * 8 + c%8,   C % 8 == 0
//
// -- the [k/8][n][8] slot form in which all three kernels stage activations in LDS.  Entry point: frtm_conv2d_act; the all-fp32 case goes to
// frtm_conv2d and its kernels, which never meet a bf16 tensor.
//
// ONLY the staging of the activation, the residual read and the final store differ from the parent kernel.  The K loop is the parent's, line for
// line: the same chunks, taps and k-steps of 16 in the same order from a zero accumulator, zeros for absent channels and for positions outside the
// image, the same LDS images and fragment reads, and the fp32 epilogue in the parent's order (scale and shift, then the residual, then ReLU).  So
//   * a bf16 input changes no bit: the parent rounds its fp32 input to bf16 (nearest even) on the way to LDS, and rounding a bf16 value is the identity
//     -- staging becomes a 16-byte copy per 8-channel slice instead of eight dword loads and a conversion;
//   * a bf16 residual is the parent's result on the residual widened to fp32 (exact);
//   * a bf16 output is the parent's fp32 result rounded to nearest even ((__bf16)v: v_cvt_pk_bf16_f32, the conversion used on load; NaN stays NaN, Inf
//     stays Inf).
// The C/D layout of the 32x32 MFMA gives a lane four consecutive channels (reg & 3) of one pixel per register group, inside ONE 8-channel slice
// (the fragment's first row is a multiple of 32, the lane half adds 4): one 8-byte store, and one 8-byte residual load, per group.  Cout % 8 == 0
// makes a group entirely inside or entirely outside the tensor.
//
// Tile forms, LDS, occupancy: the parent's (both forms of each kernel, bit-identical to each other).  The input format is a template parameter (it
// changes the staging registers of the K loop); the residual and output formats are wave-uniform branches of the epilogue.  No scratch, no spills,
// no atomics.
#include "conv_common.h"
#include "../../include/frtm_hip.h"
#include <atomic>
#include <type_traits>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

void frtm_bf16x1_count_launch();          // the per-layout launch counters of the parent units
void frtm_bf16x1_3x3_count_launch();
void frtm_bf16x1_3x3s2_count_launch();

namespace {

// p.in / p.residual / p.out point at fp32 NCHW or at the bf16 layout, as the formats say (in: the kernel's template parameter)
struct ActParams : ConvParams { int res_fmt = 0, out_fmt = 0; };

__device__ __forceinline__ u32x4 to_bf16x8(const float* v) {
  bf16x8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (__bf16)v[j];
  return __builtin_bit_cast(u32x4, h);
}
// four consecutive channels of one pixel: 8 bytes of the bf16 layout (channel c % 8 = 0 at the lowest address)
__device__ __forceinline__ u32x2 to_bf16x4(const float* v) {
  bf16x4 h;
#pragma unroll
  for (int j = 0; j < 4; ++j) h[j] = (__bf16)v[j];
  return __builtin_bit_cast(u32x2, h);
}
__device__ __forceinline__ void from_bf16x4(u32x2 w, float* v) {       // exact: a bf16 is the upper half of its fp32
  v[0] = __builtin_bit_cast(float, w[0] << 16);
  v[1] = __builtin_bit_cast(float, w[0] & 0xffff0000u);
  v[2] = __builtin_bit_cast(float, w[1] << 16);
  v[3] = __builtin_bit_cast(float, w[1] & 0xffff0000u);
}
__device__ __forceinline__ u32x4 buf_ld16s(__amdgpu_buffer_rsrc_t r, unsigned byte_off, unsigned uniform_off) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, (int)uniform_off, 0));
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// 1x1, stride 1 (k_conv1x1_bf16x1 of conv_bf16x1.hip).  IF = 1: the lane's column is one 16-byte slot per 8-channel slice.
// ---------------------------------------------------------------------------------------------------------------------------------------------
template <int BM, int BN, int YKC, int IF>
__global__ __launch_bounds__(256) void k_conv1x1_act(ActParams p) {
  constexpr int YKB = YKC / 8, YKS = YKC / 16;
  constexpr int FM = BM / 64, FN = BN / 64;
  constexpr int XG = BN / 64;
  constexpr int XK = YKB * XG / 4;
  constexpr int WQ = YKB * BM / 256;
  __shared__ __attribute__((aligned(16))) u32x4 As[2][YKB * BM], Bs[2][YKB * BN];     // [stage][k/8][row] x 16 bytes
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int mt = (p.M + BM - 1) / BM, nb = mt * ((p.Ntot + BN - 1) / BN);
  int m_tile, n_tile;
  tile_order(blockIdx.x, nb, mt, p.dMt, m_tile, n_tile);
  const int m0 = m_tile * BM, n0 = n_tile * BN;
  const int nch = (p.Cin + YKC - 1) / YKC;
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.wT, 0, (int)p.w_bytes, 0x00020000);
  const int xn = lane + 64 * (wid % XG), xkb0 = __builtin_amdgcn_readfirstlane((wid / XG) * XK);
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
  unsigned xoff = OOB;
  {
    const int n = n0 + xn;
    if (n < p.Ntot) {
      const int img = fdiv(n, p.dNpix);
      // fp32: the pixel's dword in channel 0 of its image; bf16: its 16-byte slot in slice 0 (an image is Cin / 8 slices of Npix slots)
      xoff = IF ? (unsigned)(((size_t)img * (p.Cin / 8) * p.Npix + (n - img * p.Npix)) * 16) : (unsigned)(((size_t)img * p.Cin * p.Npix + (n - img * p.Npix)) * 4);
    }
  }
  const unsigned cstride = (unsigned)p.Npix * (IF ? 16 : 4);     // bytes from one channel (fp32) / one 8-channel slice (bf16) to the next
  float xr[2][IF ? 1 : XK * 8];
  u32x4 xb[2][IF ? XK : 1];
  u32x4 wr[2][WQ];
  auto gload = [&](auto set, int c) {
    constexpr int S = decltype(set)::value;
#pragma unroll
    for (int q = 0; q < XK; ++q) {
      const int k0 = c * YKC + 8 * (xkb0 + q);
      const unsigned base = k0 < p.Cin ? xoff : OOB;            // (the absent half of a K tail reads zeros, not the next image)
      if constexpr (IF) xb[S][q] = buf_ld16s(rin, base, (unsigned)(c * YKB + xkb0 + q) * cstride);
      else {
#pragma unroll
        for (int j = 0; j < 8; ++j) xr[S][q * 8 + j] = buf_ld1s(rin, base, (unsigned)(k0 + j) * cstride);
      }
    }
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      const int e = tid + 256 * q, r = e % BM, kg = c * YKB + e / BM;                  // (kg >= Cin / 8: past the image, zeros)
      wr[S][q] = __builtin_bit_cast(u32x4, buf_ld4(rw, (unsigned)((kg * p.Mp + m0 + r) * 16)));
    }
  };
  auto lstore = [&](auto set) {
    constexpr int S = decltype(set)::value;
#pragma unroll
    for (int q = 0; q < WQ; ++q) As[S][tid + 256 * q] = wr[S][q];
#pragma unroll
    for (int q = 0; q < XK; ++q) {
      if constexpr (IF) Bs[S][(xkb0 + q) * BN + xn] = xb[S][q];
      else Bs[S][(xkb0 + q) * BN + xn] = to_bf16x8(&xr[S][q * 8]);
    }
  };
  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  auto step = [&](auto set, int c) {
    constexpr int S = decltype(set)::value;
    if (c + 2 < nch) gload(set, c + 2);
#pragma unroll
    for (int s = 0; s < YKS; ++s) {
      const int kb = 2 * s + (lane >> 5);
      bf16x8 af[FM], bf[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = __builtin_bit_cast(bf16x8, As[S][kb * BM + wm * (BM / 2) + i * 32 + (lane & 31)]);
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[j] = __builtin_bit_cast(bf16x8, Bs[S][kb * BN + wn * (BN / 2) + j * 32 + (lane & 31)]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (c + 1 < nch) lstore(std::integral_constant<int, 1 - S>{});
    __syncthreads();
  };
  const std::integral_constant<int, 0> set0;
  const std::integral_constant<int, 1> set1;
  gload(set0, 0);
  if (nch > 1) gload(set1, 1);
  lstore(set0);
  __syncthreads();
  for (int c = 0; c < nch; c += 2) {
    step(set0, c);
    if (c + 1 < nch) step(set1, c + 1);
  }
  // C/D layout of the 32x32 MFMA: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  The parent's epilogue; in the
  // bf16 layout the four rows of register group g = reg >> 2 are 8 bytes at channel offset 4 (lane >> 5) of slice (mb + 8 g) / 8.
  int img[FN], rem[FN];
  bool col[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int n = n0 + wn * (BN / 2) + j * 32 + (lane & 31);
    col[j] = n < p.Ntot;
    img[j] = col[j] ? fdiv(n, p.dNpix) : 0;
    rem[j] = n - img[j] * p.Npix;
  }
  const unsigned short* resb = (const unsigned short*)p.residual;
  unsigned short* outb = (unsigned short*)p.out;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int mb = m0 + wm * (BM / 2) + i * 32 + 4 * (lane >> 5);
      float sc[16], sh[16], rs[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mb + (r & 3) + 8 * (r >> 2);
        sc[r] = (p.scale && m < p.M) ? p.scale[m] : 1.f;
        sh[r] = (p.scale && m < p.M) ? p.shift[m] : 0.f;
      }
      if (p.res_fmt) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int m = mb + 8 * g;
          u32x2 w = {0u, 0u};
          if (p.residual && col[j] && m < p.M) w = *(const u32x2*)(resb + (((size_t)img[j] * (p.M / 8) + m / 8) * p.Npix + rem[j]) * 8 + (m & 7));
          from_bf16x4(w, &rs[4 * g]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = mb + (r & 3) + 8 * (r >> 2);
          rs[r] = (p.residual && col[j] && m < p.M) ? p.residual[((size_t)img[j] * p.M + m) * p.Npix + rem[j]] : 0.f;
        }
      }
      float o[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[i][j][r];
        if (p.scale) v = v * sc[r] + sh[r];
        if (p.residual) v += rs[r];
        if (p.relu) v = fmaxf(v, 0.f);
        o[r] = v;
      }
      if (p.out_fmt) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int m = mb + 8 * g;
          if (col[j] && m < p.M) *(u32x2*)(outb + (((size_t)img[j] * (p.M / 8) + m / 8) * p.Npix + rem[j]) * 8 + (m & 7)) = to_bf16x4(&o[4 * g]);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = mb + (r & 3) + 8 * (r >> 2);
          if (col[j] && m < p.M) p.out[((size_t)img[j] * p.M + m) * p.Npix + rem[j]] = o[r];
        }
      }
      __builtin_amdgcn_sched_barrier(0);          // one fragment's batch at a time
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The epilogue of the two 3x3 kernels (k_conv3x3_bf16x1 / k_conv3x3s2_bf16x1): everything through buffer resources of exact size -- this image's
// M x Npix elements of the output and the residual in their format, the M floats of scale and shift -- with the row in the per-lane offset: a row
// past Cout or a pixel outside the image is out of range, its loads return zero and its store is dropped.  In the bf16 layout a register group is
// the 8 bytes at (slice (mb + 8 g) / 8, pixel) + 2 (mb % 8); a slice past Cout / 8 starts at or after the resource's end.
// pix: y * Wo + x of the lane's pixel, or -1 outside the image.  (The launcher checked (M + 96) Npix 4 < 2^31: no offset wraps.)
// ---------------------------------------------------------------------------------------------------------------------------------------------
template <int FM>
__device__ __forceinline__ void epilogue3x3(const ActParams& p, const f32x16 (&acc)[FM][2], int img, int m0, int h, const int (&pix)[2]) {
  const unsigned rowb = (unsigned)p.Npix * 4, img_bytes = (unsigned)p.M * rowb;
  const size_t img_off = (size_t)img * p.M * p.Npix;                       // elements of either format
  const __amdgpu_buffer_rsrc_t rout = p.out_fmt ? __builtin_amdgcn_make_buffer_rsrc((void*)((unsigned short*)p.out + img_off), 0, (int)(img_bytes / 2), 0x00020000)
                                                : __builtin_amdgcn_make_buffer_rsrc((void*)(p.out + img_off), 0, (int)img_bytes, 0x00020000);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const unsigned pb = pix[j] >= 0 ? (unsigned)pix[j] * 4 : OOB;          // fp32: the pixel's dword in row 0
    const unsigned pb16 = pix[j] >= 0 ? (unsigned)pix[j] * 16 : OOB;       // bf16: its slot in slice 0
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int mb = m0 + i * 32 + 4 * h;
      const unsigned vo = pb + (unsigned)mb * rowb;
      const unsigned vo16 = pb16 + (unsigned)(mb / 8) * (rowb * 4) + 8 * h;
      float sc[16], sh[16], rs[16];
      if (p.scale) {
        const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc((void*)p.scale, 0, p.M * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsh = __builtin_amdgcn_make_buffer_rsrc((void*)p.shift, 0, p.M * 4, 0x00020000);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sc[r] = buf_ld1(rsc, (unsigned)(mb + (r & 3) + 8 * (r >> 2)) * 4);
          sh[r] = buf_ld1(rsh, (unsigned)(mb + (r & 3) + 8 * (r >> 2)) * 4);
        }
      }
      if (p.residual) {
        if (p.res_fmt) {
          const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc((void*)((const unsigned short*)p.residual + img_off), 0, (int)(img_bytes / 2), 0x00020000);
#pragma unroll
          for (int g = 0; g < 4; ++g) from_bf16x4(__builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rres, (int)(vo16 + (unsigned)g * (rowb * 4)), 0, 0)), &rs[4 * g]);
        } else {
          const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc((void*)(p.residual + img_off), 0, (int)img_bytes, 0x00020000);
#pragma unroll
          for (int r = 0; r < 16; ++r) rs[r] = buf_ld1(rres, vo + (unsigned)((r & 3) + 8 * (r >> 2)) * rowb);
        }
      }
      float o[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[i][j][r];
        if (p.scale) v = v * sc[r] + sh[r];
        if (p.residual) v += rs[r];
        if (p.relu) v = fmaxf(v, 0.f);
        o[r] = v;
      }
      if (p.out_fmt) {
#pragma unroll
        for (int g = 0; g < 4; ++g) __builtin_amdgcn_raw_buffer_store_b64(to_bf16x4(&o[4 * g]), rout, (int)(vo16 + (unsigned)g * (rowb * 4)), 0, 0);
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, o[r]), rout, (int)(vo + (unsigned)((r & 3) + 8 * (r >> 2)) * rowb), 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);          // one fragment's batch at a time
    }
  }
}

constexpr int TH = 8, TW = 32;                          // output tile of a workgroup (both 3x3 kernels)
constexpr int KC = 16;                                  // channels per chunk = K of one MFMA

// ---------------------------------------------------------------------------------------------------------------------------------------------
// 3x3, pad 1, stride 1 (k_conv3x3_bf16x1 of conv3x3_bf16x1.hip).  IF = 1: a patch position is one 16-byte slot per 8-channel slice, two per chunk;
// Cin % 16 == 8 leaves the second slice of the last chunk absent (zeros, as the parent loads its absent channels).
// ---------------------------------------------------------------------------------------------------------------------------------------------
namespace s1 {
constexpr int PH = TH + 2, PW = TW + 2, PP = PH * PW;   // the input patch of a tile
constexpr int XQ = (PP + 255) / 256;                    // patch positions per thread
}

template <int FM, int IF>
__global__ __launch_bounds__(256, 2) void k_conv3x3_act(ActParams p) {
  using namespace s1;
  constexpr int BM = 32 * FM;
  constexpr int WE = 18 * BM, WQ = (WE + 255) / 256;
  __shared__ __attribute__((aligned(16))) u32x4 As[2][WE], Bs[2][2 * PP];        // [stage][tap * 2 + g][row] and [stage][g][patch row][patch col]
  const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int mt = (p.M + BM - 1) / BM;
  const int tx = (p.Wo + TW - 1) / TW, ty = (p.Ho + TH - 1) / TH;
  const int nb = mt * p.B * ty * tx;
  int m_tile, n_tile;
  tile_order(blockIdx.x, nb, mt, p.dMt, m_tile, n_tile);
  const int m0 = m_tile * BM;
  const int img = fdiv(n_tile, p.dA), t_in = n_tile - img * (ty * tx);
  const int tyi = fdiv(t_in, p.dB), txi = t_in - tyi * tx;
  const int y0 = tyi * TH, x0 = txi * TW;
  const int nch = (p.Cin + KC - 1) / KC;
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.wT, 0, (int)p.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
  unsigned xoff[XQ];
#pragma unroll
  for (int q = 0; q < XQ; ++q) {
    const int pos = tid + 256 * q, pr = pos / PW, pc = pos - pr * PW;
    const int gy = y0 - 1 + pr, gx = x0 - 1 + pc;
    const bool ok = pos < PP && gy >= 0 && gy < p.Hin && gx >= 0 && gx < p.Win;
    const size_t at = (size_t)gy * p.Win + gx;
    xoff[q] = !ok ? OOB : IF ? (unsigned)(((size_t)img * (p.Cin / 8) * p.Npix + at) * 16) : (unsigned)(((size_t)img * p.Cin * p.Npix + at) * 4);
  }
  unsigned woff[WQ];
#pragma unroll
  for (int q = 0; q < WQ; ++q) {
    const int e = tid + 256 * q, tg = e / BM, r = e - tg * BM;
    woff[q] = (e < WE && m0 + r < p.Mp) ? (unsigned)((tg * p.Mp + m0 + r) * 16) : OOB;
  }
  const unsigned cstride = (unsigned)p.Npix * (IF ? 16 : 4);    // bytes from one channel (fp32) / one 8-channel slice (bf16) to the next
  const unsigned wstride = (unsigned)p.Mp * (18 * 16);
  float xr[IF ? 1 : XQ][16];
  u32x4 xb[IF ? XQ : 1][2];
  u32x4 wr[WQ];
  auto gload = [&](int c) {
    if constexpr (IF) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const unsigned absent = (2 * c + g) * 8 < p.Cin ? 0u : OOB;           // the slice exists (uniform)
#pragma unroll
        for (int q = 0; q < XQ; ++q) xb[q][g] = buf_ld16s(rin, xoff[q] | absent, (unsigned)(2 * c + g) * cstride);
      }
    } else {
      const int nv = p.Cin - c * KC;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const unsigned absent = (unsigned)(nv - 1 - k) & OOB;
#pragma unroll
        for (int q = 0; q < XQ; ++q) xr[q][k] = buf_ld1s(rin, xoff[q] | absent, (unsigned)(c * KC + k) * cstride);
      }
    }
#pragma unroll
    for (int q = 0; q < WQ; ++q) wr[q] = __builtin_bit_cast(u32x4, buf_ld4s(rw, woff[q], (unsigned)c * wstride));
  };
  auto lstore = [&](int S) {
#pragma unroll
    for (int q = 0; q < WQ; ++q)
      if (tid + 256 * q < WE) As[S][tid + 256 * q] = wr[q];
#pragma unroll
    for (int q = 0; q < XQ; ++q)
      if (tid + 256 * q < PP) {
        if constexpr (IF) {
          Bs[S][tid + 256 * q] = xb[q][0];
          Bs[S][PP + tid + 256 * q] = xb[q][1];
        } else {
          Bs[S][tid + 256 * q] = to_bf16x8(&xr[q][0]);
          Bs[S][PP + tid + 256 * q] = to_bf16x8(&xr[q][8]);
        }
      }
  };
  f32x16 acc[FM][2];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int abase = h * BM + l31, bbase = h * PP + 2 * wn * PW + l31;
  gload(0);
  lstore(0);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const int S = c & 1;
    if (c + 1 < nch) gload(c + 1);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kh = tap / 3, kw = tap - 3 * kh;
      bf16x8 af[FM], bf[2];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = __builtin_bit_cast(bf16x8, As[S][abase + tap * 2 * BM + i * 32]);
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = __builtin_bit_cast(bf16x8, Bs[S][bbase + (j + kh) * PW + kw]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (c + 1 < nch) lstore(1 - S);
    __syncthreads();
  }
  const int x = x0 + l31;
  int pix[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int y = y0 + 2 * wn + j;
    pix[j] = (y < p.Ho && x < p.Wo) ? y * p.Wo + x : -1;
  }
  epilogue3x3<FM>(p, acc, img, m0, h, pix);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// 3x3, pad 1, stride 2 (k_conv3x3s2_bf16x1 of conv3x3s2_bf16x1.hip): one LDS stage, patch rows split by column parity, two barriers per chunk.
// ---------------------------------------------------------------------------------------------------------------------------------------------
namespace s2 {
constexpr int PH = 2 * TH + 1, PW = 2 * TW + 1, PP = PH * PW;   // the input patch of a tile: 17 x 65
constexpr int NE = TW + 1;                                      // even columns of a patch row (slots 0 .. 32; the odd ones follow)
constexpr int XQ = (PP + 255) / 256;
}

template <int FM, int IF>
__global__ __launch_bounds__(256, 2) void k_conv3x3s2_act(ActParams p) {
  using namespace s2;
  constexpr int BM = 32 * FM;
  constexpr int WE = 18 * BM, WQ = (WE + 255) / 256;
  __shared__ __attribute__((aligned(16))) u32x4 As[WE], Bs[2 * PP];        // [tap * 2 + g][row] and [g][patch row][slot]
  const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int mt = (p.M + BM - 1) / BM;
  const int tx = (p.Wo + TW - 1) / TW, ty = (p.Ho + TH - 1) / TH;
  const int nb = mt * p.B * ty * tx;
  int m_tile, n_tile;
  tile_order(blockIdx.x, nb, mt, p.dMt, m_tile, n_tile);
  const int m0 = m_tile * BM;
  const int img = fdiv(n_tile, p.dA), t_in = n_tile - img * (ty * tx);
  const int tyi = fdiv(t_in, p.dB), txi = t_in - tyi * tx;
  const int y0 = tyi * TH, x0 = txi * TW;
  const int nch = (p.Cin + KC - 1) / KC;
  const int in_pix = p.Hin * p.Win;
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.wT, 0, (int)p.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
  unsigned xoff[XQ];
#pragma unroll
  for (int q = 0; q < XQ; ++q) {
    const int pos = tid + 256 * q, pr = pos / PW, s = pos - pr * PW;
    const int pc = s < NE ? 2 * s : 2 * (s - NE) + 1;
    const int gy = 2 * y0 - 1 + pr, gx = 2 * x0 - 1 + pc;
    const bool ok = pos < PP && gy >= 0 && gy < p.Hin && gx >= 0 && gx < p.Win;
    const size_t at = (size_t)gy * p.Win + gx;
    xoff[q] = !ok ? OOB : IF ? (unsigned)(((size_t)img * (p.Cin / 8) * in_pix + at) * 16) : (unsigned)(((size_t)img * p.Cin * in_pix + at) * 4);
  }
  unsigned woff[WQ];
#pragma unroll
  for (int q = 0; q < WQ; ++q) {
    const int e = tid + 256 * q, tg = e / BM, r = e - tg * BM;
    woff[q] = (e < WE && m0 + r < p.Mp) ? (unsigned)((tg * p.Mp + m0 + r) * 16) : OOB;
  }
  const unsigned cstride = (unsigned)in_pix * (IF ? 16 : 4);    // bytes from one input channel (fp32) / 8-channel slice (bf16) to the next
  const unsigned wstride = (unsigned)p.Mp * (18 * 16);
  float xr[IF ? 1 : XQ][16];
  u32x4 xb[IF ? XQ : 1][2];
  u32x4 wr[WQ];
  auto gload = [&](int c) {
    if constexpr (IF) {
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        const unsigned absent = (2 * c + g) * 8 < p.Cin ? 0u : OOB;
#pragma unroll
        for (int q = 0; q < XQ; ++q) xb[q][g] = buf_ld16s(rin, xoff[q] | absent, (unsigned)(2 * c + g) * cstride);
      }
    } else {
      const int nv = p.Cin - c * KC;
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const unsigned absent = (unsigned)(nv - 1 - k) & OOB;
#pragma unroll
        for (int q = 0; q < XQ; ++q) xr[q][k] = buf_ld1s(rin, xoff[q] | absent, (unsigned)(c * KC + k) * cstride);
      }
    }
#pragma unroll
    for (int q = 0; q < WQ; ++q) wr[q] = __builtin_bit_cast(u32x4, buf_ld4s(rw, woff[q], (unsigned)c * wstride));
  };
  auto lstore = [&]() {
#pragma unroll
    for (int q = 0; q < WQ; ++q)
      if (tid + 256 * q < WE) As[tid + 256 * q] = wr[q];
#pragma unroll
    for (int q = 0; q < XQ; ++q)
      if (tid + 256 * q < PP) {
        if constexpr (IF) {
          Bs[tid + 256 * q] = xb[q][0];
          Bs[PP + tid + 256 * q] = xb[q][1];
        } else {
          Bs[tid + 256 * q] = to_bf16x8(&xr[q][0]);
          Bs[PP + tid + 256 * q] = to_bf16x8(&xr[q][8]);
        }
      }
  };
  f32x16 acc[FM][2];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int abase = h * BM + l31, bbase = h * PP + 4 * wn * PW + l31;       // (output rows 2 wn + j: patch rows 2 (2 wn + j) + kh)
  gload(0);
  lstore();
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) gload(c + 1);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int kh = tap / 3, kw = tap - 3 * kh;
      const int ks = kw == 1 ? NE : kw >> 1;
      bf16x8 af[FM], bf[2];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = __builtin_bit_cast(bf16x8, As[abase + tap * 2 * BM + i * 32]);
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = __builtin_bit_cast(bf16x8, Bs[bbase + (2 * j + kh) * PW + ks]);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (c + 1 < nch) {                  // (uniform: every thread of the workgroup takes both barriers or neither)
      __syncthreads();
      lstore();
      __syncthreads();
    }
  }
  const int x = x0 + l31;
  int pix[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int y = y0 + 2 * wn + j;
    pix[j] = (y < p.Ho && x < p.Wo) ? y * p.Wo + x : -1;
  }
  epilogue3x3<FM>(p, acc, img, m0, h, pix);
}

std::atomic<long> g_bf16act_launches{0};

int cu_count() {
  static const int N = [] {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess) (void)hipGetLastError();
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
    return cus;
  }();
  return N;
}

template <int BM, int IF>
int launch1x1(ActParams p, hipStream_t st) {
  fill_divs(p, BM);
  const long nb = (long)((p.M + BM - 1) / BM) * ((p.Ntot + 63) / 64);
  FRTM_CHECK_ARG(nb < 0x7fffffffL, "frtm_conv2d_act: too many tiles");
  k_conv1x1_act<BM, 64, 64, IF><<<(int)nb, 256, 0, st>>>(p);
  conv_trace("k_conv1x1_act<%d,64,64,%d>", BM, IF);
  FRTM_LAUNCH_CHECK();
  frtm_bf16x1_count_launch();
  g_bf16act_launches += 1;
  return FRTM_OK;
}

template <int FM, int IF>
int launch3x3(ActParams p, int stride, hipStream_t st) {
  constexpr int BM = 32 * FM;
  fill_divs(p, BM);
  const int tx = (p.Wo + TW - 1) / TW, ty = (p.Ho + TH - 1) / TH;
  p.dA = fast_div((unsigned)(ty * tx));
  p.dB = fast_div((unsigned)tx);
  const long nb = (long)((p.M + BM - 1) / BM) * p.B * ty * tx;
  FRTM_CHECK_ARG(nb < 0x7fffffffL, "frtm_conv2d_act: too many tiles");
  FRTM_CHECK_ARG((size_t)(p.M + 96) * p.Npix * 4 < 0x7fffffffull, "frtm_conv2d_act: an output image too large for 32-bit buffer offsets");
  if (stride == 2) {
    k_conv3x3s2_act<FM, IF><<<(int)nb, 256, 0, st>>>(p);
    conv_trace("k_conv3x3s2_act<%d,%d>", FM, IF);
  } else {
    k_conv3x3_act<FM, IF><<<(int)nb, 256, 0, st>>>(p);
    conv_trace("k_conv3x3_act<%d,%d>", FM, IF);
  }
  FRTM_LAUNCH_CHECK();
  if (stride == 2) frtm_bf16x1_3x3s2_count_launch();
  else frtm_bf16x1_3x3_count_launch();
  g_bf16act_launches += 1;
  return FRTM_OK;
}

}  // namespace

extern "C" int frtm_conv2d_act(const frtm_conv_desc* d, const void* in, const float* wT, const int* ktab, const float* scale, const float* shift,
                               const void* residual, void* out, float* workspace, int in_fmt, int res_fmt, int out_fmt, frtm_stream_t stream) {
  conv_trace_reset();
  FRTM_CHECK_ARG((in_fmt == FRTM_ACT_FP32 || in_fmt == FRTM_ACT_BF16) && (res_fmt == FRTM_ACT_FP32 || res_fmt == FRTM_ACT_BF16) &&
                 (out_fmt == FRTM_ACT_FP32 || out_fmt == FRTM_ACT_BF16), "frtm_conv2d_act: a format is 0 (fp32 NCHW) or 1 (bf16, channel-blocked by 8), got %d %d %d", in_fmt, res_fmt, out_fmt);
  if (!residual) res_fmt = FRTM_ACT_FP32;                        // no residual: its format says nothing
  if (!in_fmt && !res_fmt && !out_fmt)                           // all fp32: the parent kernels
    return frtm_conv2d(d, (const float*)in, wT, ktab, scale, shift, (const float*)residual, (float*)out, workspace, stream);
  FRTM_CHECK_ARG(d && in && wT && out, "frtm_conv2d_act: null pointer");
  FRTM_CHECK_ARG(d->B > 0 && d->Cin > 0 && d->Cout > 0 && d->Hin > 0 && d->Win > 0, "frtm_conv2d_act: bad shape");
  FRTM_CHECK_ARG((scale == nullptr) == (shift == nullptr), "frtm_conv2d_act: scale and shift go together");
  const int L = d->w_layout;
  FRTM_CHECK_ARG(L == FRTM_WLAYOUT_BF16X1 || L == FRTM_WLAYOUT_BF16X1_3X3 || L == FRTM_WLAYOUT_BF16X1_3X3_S2,
                 "frtm_conv2d_act: a bf16 activation format needs one of the bf16x1 layouts 6, 7, 8 (got w_layout %d)", L);
  FRTM_CHECK_ARG(!d->out_transposed, "frtm_conv2d_act: the bf16x1 layouts write NCHW or the bf16 layout only (out_transposed is set)");
  FRTM_CHECK_ARG(d->splitk >= 0 && d->splitk <= 1, "frtm_conv2d_act: the bf16x1 layouts have no split-K (splitk %d)", d->splitk);
  FRTM_CHECK_ARG(d->w_pitch == 0, "frtm_conv2d_act: the bf16x1 layouts take their packed image only (w_pitch %d)", d->w_pitch);
  const bool one = L == FRTM_WLAYOUT_BF16X1;
  const int want_stride = L == FRTM_WLAYOUT_BF16X1_3X3_S2 ? 2 : 1;
  FRTM_CHECK_ARG(d->ksize == (one ? 1 : 3) && d->stride == want_stride && d->pad == (one ? 0 : 1),
                 "frtm_conv2d_act: layout %d needs ksize %d, stride %d, pad %d (got %d, %d, %d)", L, one ? 1 : 3, want_stride, one ? 0 : 1, d->ksize, d->stride, d->pad);
  FRTM_CHECK_ARG(!one || d->Cin % 16 == 0, "frtm_conv2d_act: the bf16x1 layout needs Cin %% 16 == 0 (got %d)", d->Cin);
  FRTM_CHECK_ARG(!in_fmt || d->Cin % 8 == 0, "frtm_conv2d_act: a bf16 input needs Cin %% 8 == 0 (got %d)", d->Cin);
  FRTM_CHECK_ARG(!(res_fmt || out_fmt) || d->Cout % 8 == 0, "frtm_conv2d_act: a bf16 residual or output needs Cout %% 8 == 0 (got %d)", d->Cout);
  FRTM_CHECK_ARG(((size_t)wT) % 16 == 0 && (!in_fmt || ((size_t)in) % 16 == 0) && (!res_fmt || ((size_t)residual) % 16 == 0) && (!out_fmt || ((size_t)out) % 16 == 0),
                 "frtm_conv2d_act: the weight image and every bf16 tensor must be 16-byte aligned");
  FRTM_CHECK_ARG(d->tile >= 0 && d->tile <= 2, "frtm_conv2d_act: tile selects the parent's form (0 auto, 1, 2), got %d", d->tile);
  ActParams p;
  p.in = (const float*)in; p.wT = wT; p.ktab = nullptr; p.scale = scale; p.shift = shift; p.residual = (const float*)residual; p.out = (float*)out; p.ws = nullptr;
  p.B = d->B; p.Cin = d->Cin; p.Hin = d->Hin; p.Win = d->Win; p.M = d->Cout; p.stride = d->stride; p.pad = d->pad;
  p.Ho = (d->Hin + 2 * d->pad - d->ksize) / d->stride + 1;
  p.Wo = (d->Win + 2 * d->pad - d->ksize) / d->stride + 1;
  FRTM_CHECK_ARG(p.Ho > 0 && p.Wo > 0, "frtm_conv2d_act: empty output");
  p.K = d->Cin * d->ksize * d->ksize;
  p.Npix = p.Ho * p.Wo;
  p.Ntot = d->B * p.Npix;
  p.relu = d->relu; p.out_transposed = 0; p.splitk = 1;
  p.res_fmt = res_fmt; p.out_fmt = out_fmt;
  const size_t in_bytes = (size_t)d->B * d->Cin * d->Hin * d->Win * (in_fmt ? 2 : 4);
  FRTM_CHECK_ARG(in_bytes < 0x7fffffffull && (size_t)d->B * d->Cin * d->Hin * d->Win * 4 < 0x7fffffffull, "frtm_conv2d_act: tensor too large for 32-bit buffer offsets");
  p.in_bytes = (unsigned)in_bytes;
  hipStream_t st = (hipStream_t)stream;
  int tile = d->tile;
  if (one) {                                                    // frtm_bf16x1_launch's image size and automatic form
    p.Mp = (p.M + 127) / 128 * 128;
    p.w_bytes = (unsigned)((size_t)p.Cin * p.Mp * 2);
    FRTM_CHECK_ARG((size_t)p.Cin * p.Mp * 2 < 0x7fffffffull, "frtm_conv2d_act: weight image too large for 32-bit buffer offsets");
    p.nchunks = p.chunks_per_split = (p.Cin + 63) / 64;
    if (tile == 0) {
      const long big = (long)((p.M + 127) / 128) * ((p.Ntot + 63) / 64);
      tile = (p.Cin >= 1024 && big >= cu_count()) ? FRTM_BF16X1_TILE_128x64 : FRTM_BF16X1_TILE_64x64;
    }
    if (tile == FRTM_BF16X1_TILE_128x64) return in_fmt ? launch1x1<128, 1>(p, st) : launch1x1<128, 0>(p, st);
    return in_fmt ? launch1x1<64, 1>(p, st) : launch1x1<64, 0>(p, st);
  }
  p.Mp = (p.M + 31) / 32 * 32;                                  // frtm_bf16x1_3x3_launch's
  const size_t w_bytes = (size_t)((p.Cin + KC - 1) / KC) * 18 * p.Mp * 16;
  FRTM_CHECK_ARG(w_bytes < 0x7fffffffull, "frtm_conv2d_act: weight image too large for 32-bit buffer offsets");
  p.w_bytes = (unsigned)w_bytes;
  if (tile == 0) tile = 3 * ((p.M + 95) / 96) < 2 * ((p.M + 63) / 64) ? FRTM_BF16X1_3X3_TILE_96 : FRTM_BF16X1_3X3_TILE_64;
  if (tile == FRTM_BF16X1_3X3_TILE_96) return in_fmt ? launch3x3<3, 1>(p, d->stride, st) : launch3x3<3, 0>(p, d->stride, st);
  return in_fmt ? launch3x3<2, 1>(p, d->stride, st) : launch3x3<2, 0>(p, d->stride, st);
}

extern "C" long frtm_conv_bf16act_launches(void) { return g_bf16act_launches.load(); }
