// bf16x1 3x3 STRIDE-2 convolution (opt-in bf16x1_3x3 trunk mode, FRTM_WLAYOUT_BF16X1_3X3_S2): pad 1 (zeros), NCHW fp32 in and out, any Cin, Cout, B, H, W;
// Ho = (Hin - 1) / 2 + 1, Wo = (Win - 1) / 2 + 1.  The convs that open a ResNet stage (three per trunk).
//
//   out[img, m, y, x] = epilogue( sum_{ci,kh,kw} bf16(W[m,ci,kh,kw]) * bf16(X[img, ci, 2y-1+kh, 2x-1+kw]) )     epilogue as frtm_conv2d, in fp32
//
// Arithmetic, semantics and weight image are those of conv3x3_bf16x1.hip (FRTM_WLAYOUT_BF16X1_3X3), byte for byte the same image (packed by that file's
// kernel): operands rounded to bf16 once, to nearest even (the weights at pack time, the activations on their way to LDS), v_mfma_f32_32x32x16_bf16,
// fp32 accumulation and epilogue.  Every output element is one fixed sequence of MFMAs from a zero accumulator -- chunks of 16 channels ascending, the
// nine taps ascending inside a chunk -- so the result is deterministic and independent of the tile form, the grid and the batch size; no atomics.
// Padding is zeros on both operands: channels past Cin and positions outside the image are loaded as zeros, never as the next image's data.
//
// A workgroup (four waves) computes BM output channels x 8 rows x 32 columns of one image; a wave owns two output rows and all BM channels (FM x 2
// fragments of 32 x 32).  Per chunk of 16 channels the raw 17 x 65 input patch is staged once as bf16, [g = 8-channel group][patch row][65 slots of
// 16 bytes]: 35,360 bytes.  A tap's 32-pixel fragment reads every SECOND patch column, which as 16-byte slots at a 32-byte pitch would put lanes l and
// l + 8 of a ds_read_b128 lane group on the same banks (2-way).  So a patch row is stored SPLIT BY COLUMN PARITY: slots 0 .. 32 hold the even patch
// columns 0, 2, .. 64, slots 33 .. 64 the odd ones 1, 3, .. 63.  Tap column kw = 0 reads slots lx, kw = 1 slots 33 + lx, kw = 2 slots 1 + lx: every
// fragment read is 32 consecutive slots, conflict-free like the stride-1 kernel's.  The staging threads are numbered in SLOT order (consecutive
// threads write consecutive slots; their global loads are dwords 8 bytes apart inside a row).
//
// LDS: ONE stage of the patch (35,360 B) and ONE of the chunk's 18 x BM weight slices (18,432 B at BM = 64, 27,648 B at BM = 96): 53.8 / 63.0 KB,
// TWO workgroups per CU (a second patch stage would make it 107 / 126 KB: one).  The global loads of chunk c + 1 are requested into registers before
// the MFMAs of chunk c; after them a barrier frees the stage, the registers are converted and stored, a second barrier publishes it.  The other
// workgroup of the CU computes meanwhile.  222 (BM = 64) / 248 (BM = 96) VGPRs: two waves per SIMD; no scratch, no spills.
//
// Tile forms (frtm_conv_desc.tile; 0 = automatic: fewer padded rows, the small one on a tie), bit-identical to each other, as in layout 7:
//   1  FRTM_BF16X1_3X3_TILE_64   BM = 64 (FM = 2)
//   2  FRTM_BF16X1_3X3_TILE_96   BM = 96 (FM = 3)
#include "conv_common.h"
#include "../../include/frtm_hip.h"
#include <atomic>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int TH = 8, TW = 32;                                  // output tile of a workgroup
constexpr int PH = 2 * TH + 1, PW = 2 * TW + 1, PP = PH * PW;   // its input patch: 17 x 65
constexpr int NE = TW + 1;                                      // even columns of a patch row (slots 0 .. 32; the odd ones follow)
constexpr int XQ = (PP + 255) / 256;                            // patch positions per thread
constexpr int KC = 16;                                          // channels per chunk = K of one MFMA

__device__ __forceinline__ u32x4 to_bf16x8(const float* v) {
  bf16x8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (__bf16)v[j];
  return __builtin_bit_cast(u32x4, h);
}

template <int FM>
__global__ __launch_bounds__(256, 2) void k_conv3x3s2_bf16x1(ConvParams p) {
  constexpr int BM = 32 * FM;
  constexpr int WE = 18 * BM, WQ = (WE + 255) / 256;     // 16-byte weight entries per chunk, per thread
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
  // activation staging: this thread fills LDS slots tid + 256 q of each 8-channel group; slot s of patch row pr holds patch column 2 s (s <= 32) or
  // 2 (s - 33) + 1.  A position outside the image (the zero padding, the overhang of an edge tile) or past the patch reads zeros
  unsigned xoff[XQ];
#pragma unroll
  for (int q = 0; q < XQ; ++q) {
    const int pos = tid + 256 * q, pr = pos / PW, s = pos - pr * PW;
    const int pc = s < NE ? 2 * s : 2 * (s - NE) + 1;
    const int gy = 2 * y0 - 1 + pr, gx = 2 * x0 - 1 + pc;
    const bool ok = pos < PP && gy >= 0 && gy < p.Hin && gx >= 0 && gx < p.Win;
    xoff[q] = ok ? (unsigned)(((size_t)img * p.Cin * in_pix + (size_t)gy * p.Win + gx) * 4) : OOB;
  }
  // weight staging: entries tid + 256 q of the chunk's [18][BM] slice; rows past the image's Mp (an M tile's overhang) read zeros
  unsigned woff[WQ];
#pragma unroll
  for (int q = 0; q < WQ; ++q) {
    const int e = tid + 256 * q, tg = e / BM, r = e - tg * BM;
    woff[q] = (e < WE && m0 + r < p.Mp) ? (unsigned)((tg * p.Mp + m0 + r) * 16) : OOB;
  }
  const unsigned cstride = (unsigned)in_pix * 4;          // bytes from one input channel to the next
  const unsigned wstride = (unsigned)p.Mp * (18 * 16);    // ... and from one chunk of the weight image to the next
  float xr[XQ][16];
  u32x4 wr[WQ];
  auto gload = [&](int c) {
    const int nv = p.Cin - c * KC;                        // channels of this chunk that exist (the others read zeros, never the next image)
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const unsigned absent = (unsigned)(nv - 1 - k) & OOB;        // the sign bit as an offset: OOB for k >= nv
#pragma unroll
      for (int q = 0; q < XQ; ++q) xr[q][k] = buf_ld1s(rin, xoff[q] | absent, (unsigned)(c * KC + k) * cstride);
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
        Bs[tid + 256 * q] = to_bf16x8(&xr[q][0]);
        Bs[PP + tid + 256 * q] = to_bf16x8(&xr[q][8]);
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
      const int ks = kw == 1 ? NE : kw >> 1;              // first slot of the tap's fragment: even columns from 0 or 1, odd columns from 33
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
      __syncthreads();                  // every wave has read chunk c
      lstore();
      __syncthreads();
    }
  }
  // C/D layout of the 32x32 MFMA: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  The epilogue of
  // k_conv3x3_bf16x1: everything goes through buffer resources of exact size -- this image's M x Npix floats of the output and the residual, the M
  // floats of scale and shift -- with the row in the per-lane offset: a row past Cout or a pixel outside the image is out of range, its loads return
  // zero and its store is dropped.
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

std::atomic<long> g_bf16x1_3x3s2_launches{0};

template <int FM>
int launch_form(ConvParams p, hipStream_t st) {
  constexpr int BM = 32 * FM;
  fill_divs(p, BM);
  const int tx = (p.Wo + TW - 1) / TW, ty = (p.Ho + TH - 1) / TH;
  p.dA = fast_div((unsigned)(ty * tx));
  p.dB = fast_div((unsigned)tx);
  const long nb = (long)((p.M + BM - 1) / BM) * p.B * ty * tx;
  FRTM_CHECK_ARG(nb < 0x7fffffffL, "frtm_conv2d: too many tiles");
  FRTM_CHECK_ARG((size_t)(p.M + 96) * p.Npix * 4 < 0x7fffffffull, "frtm_conv2d: bf16x1 3x3 stride-2 layout: an output image too large for 32-bit buffer offsets");
  k_conv3x3s2_bf16x1<FM><<<(int)nb, 256, 0, st>>>(p);
  conv_trace("k_conv3x3s2_bf16x1<%d>", FM);
  FRTM_LAUNCH_CHECK();
  g_bf16x1_3x3s2_launches += 1;
  return FRTM_OK;
}

}  // namespace

// p as frtm_conv2d filled it for a 3x3 stride-2 pad-1 conv; p.wT = the FRTM_WLAYOUT_BF16X1_3X3 image; tile: 0 = automatic, else FRTM_BF16X1_3X3_TILE_*
int frtm_bf16x1_3x3s2_launch(ConvParams p, int tile, hipStream_t st) {
  FRTM_CHECK_ARG(((size_t)p.wT) % 16 == 0, "frtm_conv2d: the bf16x1 3x3 stride-2 image must be 16-byte aligned");
  FRTM_CHECK_ARG(tile >= 0 && tile <= FRTM_BF16X1_3X3_TILE_96, "frtm_conv2d: bf16x1 3x3 stride-2 layout: tile selects the form (0 auto, 1 64 rows, 2 96 rows), got %d", tile);
  p.Mp = (p.M + 31) / 32 * 32;
  const size_t w_bytes = (size_t)((p.Cin + KC - 1) / KC) * 18 * p.Mp * 16;
  FRTM_CHECK_ARG(w_bytes < 0x7fffffffull, "frtm_conv2d: bf16x1 3x3 stride-2 image too large for 32-bit buffer offsets");
  p.w_bytes = (unsigned)w_bytes;
  p.splitk = 1;
  if (tile == 0) tile = 3 * ((p.M + 95) / 96) < 2 * ((p.M + 63) / 64) ? FRTM_BF16X1_3X3_TILE_96 : FRTM_BF16X1_3X3_TILE_64;
  return tile == FRTM_BF16X1_3X3_TILE_96 ? launch_form<3>(p, st) : launch_form<2>(p, st);
}

extern "C" long frtm_conv_bf16x1_3x3s2_launches(void) { return g_bf16x1_3x3s2_launches.load(); }
// a launch of this layout's format-aware form (csrc/conv_bf16act.hip) counts here as well
void frtm_bf16x1_3x3s2_count_launch() { g_bf16x1_3x3s2_launches += 1; }
