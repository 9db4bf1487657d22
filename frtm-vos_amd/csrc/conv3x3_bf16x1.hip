// bf16x1 3x3 convolution (opt-in refiner precision mode, FRTM_WLAYOUT_BF16X1_3X3): stride 1, pad 1 (zeros), NCHW fp32 in and out, any Cin, Cout, B, H, W.
//
//   out[img, m, y, x] = epilogue( sum_{ci,kh,kw} bf16(W[m,ci,kh,kw]) * bf16(X[img, ci, y-1+kh, x-1+kw]) )     epilogue as frtm_conv2d, in fp32
//
// The arithmetic of conv_bf16x1.hip in the direct 3x3 form: each operand is rounded to bf16 once, to nearest even (v_cvt_pk_bf16_f32: the weights
// at pack time, the activations in registers on their way to LDS), the products run on v_mfma_f32_32x32x16_bf16, accumulation and epilogue are fp32.
// The two roundings cost up to 2^-7 of |W| conv |X| per output element; this is NOT fp32-level arithmetic.
//
// Semantics as there.  A NaN stays a NaN, an Inf stays an Inf.  The result is deterministic and does not depend on the tile form or the grid: every
// output element is the same fixed sequence of MFMAs from a zero accumulator -- channel chunks of 16 in ascending order, inside a chunk the nine taps
// (kh, kw) in ascending order, one k-step (K = 16 channels of one tap) each -- and an element of a 32x32x16 product depends on its own row and column
// of the operands only.  Padding is zeros on BOTH operands: the channels past Cin of the last chunk are zero in the weight image and are loaded as
// zeros from the activations (never the next image's data), positions outside the image are loaded as zeros, so a padded k adds +0 and a NaN
// activation never meets a padded weight in an element that is stored (rows past Cout of a tile are computed and dropped).
//
// Weight image: bf16 [chunk = ci / 16][tap][g = (ci / 8) % 2][Mp][8], Mp = Cout rounded up to 32: a lane's eight k of an MFMA operand are 16
// contiguous bytes, the two 8-channel groups of a k-step are the two lane halves.  FRTM_CONV_BF16X1_3X3_ELEMS floats.
//
// A workgroup (four waves) computes BM output channels x 8 rows x 32 columns of one image.  Per chunk it stages the raw 10 x 34 input patch ONCE, as
// bf16 in [g][row][col][8] form (21.8 KB for both stages), and the chunk's 18 x BM weight slices; all nine taps read the same patch at shifted
// addresses (a 32-pixel fragment is one output row, so a tap shifts 32 consecutive 16-byte slots: no bank conflict), there is no im2col image.  A wave
// owns two output rows and all BM channels: FM x 2 fragments of 32 x 32.  Two LDS stages; the global loads of chunk c + 1 are requested into
// registers before the MFMAs of chunk c and converted / stored after them; one barrier per chunk; no branch per k-step.
//
// Tile forms (frtm_conv_desc.tile; 0 = automatic: the form with fewer padded rows, the small one on a tie), bit-identical to each other:
//   1  FRTM_BF16X1_3X3_TILE_64   BM = 64 (FM = 2)
//   2  FRTM_BF16X1_3X3_TILE_96   BM = 96 (FM = 3): Cout 65 .. 96 in one M tile (the refiner's 65-channel convs: 96 rows, not 128)
// A 16-channel chunk per k-step means Cin 65 costs five chunks (80 channels' worth of MFMAs).
#include "conv_common.h"
#include "../../include/frtm_hip.h"
#include <atomic>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TH = 8, TW = 32;                          // output tile of a workgroup
constexpr int PH = TH + 2, PW = TW + 2, PP = PH * PW;   // its input patch
constexpr int XQ = (PP + 255) / 256;                    // patch positions per thread
constexpr int KC = 16;                                  // channels per chunk = K of one MFMA

__device__ __forceinline__ u32x4 to_bf16x8(const float* v) {
  bf16x8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (__bf16)v[j];
  return __builtin_bit_cast(u32x4, h);
}

// OIHW (Cout, Cin, 3, 3) -> P[chunk][tap][g][Mp] x 8 bf16, zero padded in both directions
__global__ __launch_bounds__(256) void k_pack_weights_bf16x1_3x3(const float* __restrict__ src, int Cout, int Cin, int Mp, long total, u32x4* __restrict__ P) {
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int m = (int)(e % Mp);
    const int tg = (int)((e / Mp) % 18), c = (int)(e / ((long)Mp * 18));
    const int tap = tg >> 1, g = tg & 1;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ci = c * KC + g * 8 + j;
      v[j] = (m < Cout && ci < Cin) ? src[((size_t)m * Cin + ci) * 9 + tap] : 0.f;
    }
    P[e] = to_bf16x8(v);
  }
}

template <int FM>
__global__ __launch_bounds__(256, 2) void k_conv3x3_bf16x1(ConvParams p) {      // (two workgroups per CU: 77 KB of LDS and 206 VGPRs at FM = 3)
  constexpr int BM = 32 * FM;
  constexpr int WE = 18 * BM, WQ = (WE + 255) / 256;     // 16-byte weight entries per chunk, per thread
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
  // activation staging: this thread loads patch positions tid + 256 q, both 8-channel groups of each chunk; a position outside the image (the zero
  // padding, the overhang of an edge tile) or past the patch reads zeros
  unsigned xoff[XQ];
#pragma unroll
  for (int q = 0; q < XQ; ++q) {
    const int pos = tid + 256 * q, pr = pos / PW, pc = pos - pr * PW;
    const int gy = y0 - 1 + pr, gx = x0 - 1 + pc;
    const bool ok = pos < PP && gy >= 0 && gy < p.Hin && gx >= 0 && gx < p.Win;
    xoff[q] = ok ? (unsigned)(((size_t)img * p.Cin * p.Npix + (size_t)gy * p.Win + gx) * 4) : OOB;
  }
  // weight staging: entries tid + 256 q of the chunk's [18][BM] slice; rows past the image's Mp (an M tile's overhang) read zeros
  unsigned woff[WQ];
#pragma unroll
  for (int q = 0; q < WQ; ++q) {
    const int e = tid + 256 * q, tg = e / BM, r = e - tg * BM;
    woff[q] = (e < WE && m0 + r < p.Mp) ? (unsigned)((tg * p.Mp + m0 + r) * 16) : OOB;
  }
  const unsigned cstride = (unsigned)p.Npix * 4;          // bytes from one channel to the next
  const unsigned wstride = (unsigned)p.Mp * (18 * 16);    // ... and from one chunk of the weight image to the next
  float xr[XQ][16];
  u32x4 wr[WQ];
  auto gload = [&](int c) {
    const int nv = p.Cin - c * KC;                        // channels of this chunk that exist (the others read zeros, never the next image)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const unsigned absent = (unsigned)(nv - 1 - k) & OOB;        // the sign bit as an offset: OOB for k >= nv (plain arithmetic: no lane mask per channel)
#pragma unroll
      for (int q = 0; q < XQ; ++q) xr[q][k] = buf_ld1s(rin, xoff[q] | absent, (unsigned)(c * KC + k) * cstride);
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
        Bs[S][tid + 256 * q] = to_bf16x8(&xr[q][0]);
        Bs[S][PP + tid + 256 * q] = to_bf16x8(&xr[q][8]);
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
  // C/D layout of the 32x32 MFMA: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  store_out's arithmetic with
  // the loads batched per fragment, as in k_conv1x1_bf16x1.  Everything goes through buffer resources of exact size -- this image's M x Npix
  // floats of the output and the residual, the M floats of scale and shift -- with the row in the per-lane offset: a row past Cout or a pixel
  // outside the image is out of range, its loads return zero and its store is dropped (no branch and no lane mask per element).
  const unsigned rowb = (unsigned)p.Npix * 4, img_bytes = (unsigned)p.M * rowb;        // (the launcher checked (M + 96) Npix 4 < 2^31: no offset wraps)
  const size_t img_off = (size_t)img * p.M * p.Npix;
  const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc((void*)(p.out + img_off), 0, (int)img_bytes, 0x00020000);
  const int x = x0 + l31;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int y = y0 + 2 * wn + j;
    const unsigned pb = (y < p.Ho && x < p.Wo) ? (unsigned)(y * p.Wo + x) * 4 : OOB;
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int mb = m0 + i * 32 + 4 * h;
      const unsigned vo = pb + (unsigned)mb * rowb;
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
        const __amdgpu_buffer_rsrc_t rres = __builtin_amdgcn_make_buffer_rsrc((void*)(p.residual + img_off), 0, (int)img_bytes, 0x00020000);
#pragma unroll
        for (int r = 0; r < 16; ++r) rs[r] = buf_ld1(rres, vo + (unsigned)((r & 3) + 8 * (r >> 2)) * rowb);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[i][j][r];
        if (p.scale) v = v * sc[r] + sh[r];
        if (p.residual) v += rs[r];
        if (p.relu) v = fmaxf(v, 0.f);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, (int)(vo + (unsigned)((r & 3) + 8 * (r >> 2)) * rowb), 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);          // one fragment's batch at a time
    }
  }
}

std::atomic<long> g_bf16x1_3x3_launches{0};

template <int FM>
int launch_form(ConvParams p, hipStream_t st) {
  constexpr int BM = 32 * FM;
  fill_divs(p, BM);
  const int tx = (p.Wo + TW - 1) / TW, ty = (p.Ho + TH - 1) / TH;
  p.dA = fast_div((unsigned)(ty * tx));
  p.dB = fast_div((unsigned)tx);
  const long nb = (long)((p.M + BM - 1) / BM) * p.B * ty * tx;
  FRTM_CHECK_ARG(nb < 0x7fffffffL, "frtm_conv2d: too many tiles");
  FRTM_CHECK_ARG((size_t)(p.M + 96) * p.Npix * 4 < 0x7fffffffull, "frtm_conv2d: bf16x1 3x3 layout: an output image too large for 32-bit buffer offsets");
  k_conv3x3_bf16x1<FM><<<(int)nb, 256, 0, st>>>(p);
  conv_trace("k_conv3x3_bf16x1<%d>", FM);
  FRTM_LAUNCH_CHECK();
  g_bf16x1_3x3_launches += 1;
  return FRTM_OK;
}

}  // namespace

int frtm_bf16x1_3x3_pack(const float* src, int Cout, int Cin, float* out, hipStream_t st) {
  FRTM_CHECK_ARG(((size_t)out) % 16 == 0, "frtm_conv_pack_weights: the bf16x1 3x3 image must be 16-byte aligned");
  const int Mp = (Cout + 31) / 32 * 32;
  const long total = (long)((Cin + KC - 1) / KC) * 18 * Mp;
  FRTM_CHECK_ARG(total * 16 < 0x7fffffffL, "frtm_conv_pack_weights: bf16x1 3x3 image too large for 32-bit buffer offsets");
  k_pack_weights_bf16x1_3x3<<<(int)std::min<long>((total + 255) / 256, 2048), 256, 0, st>>>(src, Cout, Cin, Mp, total, (u32x4*)out);
  conv_trace("k_pack_weights_bf16x1_3x3");
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

// p as frtm_conv2d filled it for a 3x3 stride-1 pad-1 conv; p.wT = the FRTM_WLAYOUT_BF16X1_3X3 image; tile: 0 = automatic, else FRTM_BF16X1_3X3_TILE_*
int frtm_bf16x1_3x3_launch(ConvParams p, int tile, hipStream_t st) {
  FRTM_CHECK_ARG(((size_t)p.wT) % 16 == 0, "frtm_conv2d: the bf16x1 3x3 image must be 16-byte aligned");
  FRTM_CHECK_ARG(tile >= 0 && tile <= FRTM_BF16X1_3X3_TILE_96, "frtm_conv2d: bf16x1 3x3 layout: tile selects the form (0 auto, 1 64 rows, 2 96 rows), got %d", tile);
  p.Mp = (p.M + 31) / 32 * 32;
  const size_t w_bytes = (size_t)((p.Cin + KC - 1) / KC) * 18 * p.Mp * 16;
  FRTM_CHECK_ARG(w_bytes < 0x7fffffffull, "frtm_conv2d: bf16x1 3x3 image too large for 32-bit buffer offsets");
  p.w_bytes = (unsigned)w_bytes;
  p.splitk = 1;
  if (tile == 0) tile = 3 * ((p.M + 95) / 96) < 2 * ((p.M + 63) / 64) ? FRTM_BF16X1_3X3_TILE_96 : FRTM_BF16X1_3X3_TILE_64;
  return tile == FRTM_BF16X1_3X3_TILE_96 ? launch_form<3>(p, st) : launch_form<2>(p, st);
}

extern "C" long frtm_conv_bf16x1_3x3_launches(void) { return g_bf16x1_3x3_launches.load(); }
// a launch of this layout's format-aware form (csrc/conv_bf16act.hip) counts here as well
void frtm_bf16x1_3x3_count_launch() { g_bf16x1_3x3_launches += 1; }
