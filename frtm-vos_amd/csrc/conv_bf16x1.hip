// bf16x1 1x1 convolution (opt-in trunk precision mode, FRTM_WLAYOUT_BF16X1): stride 1, pad 0, NCHW fp32 in and out, Cin % 16 == 0.
//
//   out[img, m, pix] = epilogue( sum_k bf16(W[m][k]) * bf16(X[img, k, pix]) )     epilogue as frtm_conv2d, in fp32: (* scale[m] + shift[m])?  (+ residual)?  relu?
//
// ONE bf16 piece per operand (conv_bf16x3.hip uses three and six piece products): each operand is rounded to bf16 once, round to nearest even
// (v_cvt_pk_bf16_f32, what (__bf16)v compiles to), the products run on v_mfma_f32_32x32x16_bf16, accumulation is fp32.  This is NOT fp32-level
// arithmetic: the two roundings cost up to 2^-7 of |W|.|X| per output element.
//
// Semantics.  A NaN stays a NaN.  An Inf stays an Inf (there is no split, so no Inf - Inf).  |v| above the largest finite bf16 (more than half a
// bf16 ulp above 0x7f7f: ~3.396e38) rounds to Inf.  Denormal operands (fp32 denormals, and values that become bf16 denormals) are whatever the
// conversion and the MFMA do with them; nothing here depends on it and the tests keep them out.  The result is deterministic, and it does NOT depend
// on the tile form or the grid: every output element is the same fixed sequence of MFMAs, k-steps of 16 in ascending order from a zero accumulator
// (the absent k-steps of a K tail multiply zeros by zeros: +0 added to an accumulator that is never -0 changes no bit), and an element of a 32x32x16
// product depends on its own row and column of the operands only.  The forms agree bit for bit.
//
// Weights are converted once, at pack time, into one bf16 plane [Cin/8][Mp][8] (Mp = Cout rounded up to 128, zero padded): a lane's eight k of an
// MFMA operand are 16 contiguous bytes.  Activations stay fp32 in HBM (producers and consumers are unchanged), are read once, converted in registers
// and staged in LDS as bf16 in the same [k/8][n][8] form.
//
// Tile forms (frtm_conv_desc.tile; 0 = automatic), both with four waves in 2 x 2, K chunks of 64:
//   1  FRTM_BF16X1_TILE_128x64   128 (Cout) x 64 (pixels), waves of 64 x 32 (2 x 1 fragments of 32 x 32): half the activation re-reads of form 2
//   2  FRTM_BF16X1_TILE_64x64    64 x 64, waves of 32 x 32: 124 VGPRs, four workgroups per CU
// Pixels are the columns of all images: tiles may straddle images, any H*W.  These launches are bound by load latency and the pipeline's fill, not
// by MFMA work or bandwidth, so the small form's occupancy wins almost everywhere (profiles/bf16x1_trunk_time.txt; a 128 x 128 form with 220 VGPRs
// measured 1.0-2.0x slower than form 2 on the trunk shapes and was not kept).  Automatic: form 1 where K is deep enough to amortise the fill
// (Cin >= 1024) AND it has at least one tile per CU (1024 -> 256 at 8 frames: 24.7 against 29.6 us; at 1 frame, 52 tiles: 18.5 against 15.1 us), else form 2.
//
// K chunks of 64 (four k-steps), two LDS stages, and the global loads run TWO chunks ahead: chunk c + 2 is requested before the MFMAs of chunk c
// into one of two register sets, and chunk c + 1 (requested one iteration earlier) is converted and stored into the other LDS stage after them --
// a load has one whole iteration more to land than in the bf16x3 kernel, whose MFMA work per chunk was six times this one's.  One barrier per chunk.
// (Chunks of 32 measured 0-6 % slower.)  Cin that is no multiple of 64 ends in a partial chunk: its absent k-steps are loaded as zeros on both sides
// (buffer loads past the weight image, a byte offset beyond the activations), so the K loop has no branch per k-step.
#include "conv_common.h"
#include "../../include/frtm_hip.h"
#include <atomic>
#include <type_traits>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int YMP = 128;                    // Cout padding of the weight image (every form's tile divides it)

__device__ __forceinline__ u32x4 to_bf16x8(const float* v) {
  bf16x8 h;
#pragma unroll
  for (int j = 0; j < 8; ++j) h[j] = (__bf16)v[j];
  return __builtin_bit_cast(u32x4, h);
}

// w(m, k) = src[m * sm + k * sk] (OIHW: sm = Cin, sk = 1; the backbone's packed GEMM image [Kp][Mp32]: sm = 1, sk = Mp32) -> P[Cin/8][Mp][8]
__global__ __launch_bounds__(256) void k_pack_weights_bf16x1(const float* __restrict__ src, int Cout, int Cin, int sm, int sk, int Mp, u32x4* __restrict__ P) {
  const long total = (long)(Cin / 8) * Mp;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int m = (int)(e % Mp), kb = (int)(e / Mp);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = m < Cout ? src[(size_t)m * sm + (size_t)(kb * 8 + j) * sk] : 0.f;
    P[e] = to_bf16x8(v);
  }
}

template <int BM, int BN, int YKC>
__global__ __launch_bounds__(256) void k_conv1x1_bf16x1(ConvParams p) {
  constexpr int YKB = YKC / 8, YKS = YKC / 16;       // 8-channel groups (16-byte operand slices) and k-steps (MFMAs of K = 16) per chunk
  constexpr int FM = BM / 64, FN = BN / 64;          // 32 x 32 fragments of a wave (2 x 2 waves)
  constexpr int XG = BN / 64;                        // activation staging: groups of 64 columns, one wave each per slice
  constexpr int XK = YKB * XG / 4;                   // ... and 8-channel slices per wave and chunk
  constexpr int WQ = YKB * BM / 256;                 // weight staging: 16-byte entries per thread and chunk
  __shared__ __attribute__((aligned(16))) u32x4 As[2][YKB * BM], Bs[2][YKB * BN];     // [stage][k/8][row] x 16 bytes
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int mt = (p.M + BM - 1) / BM, nb = mt * ((p.Ntot + BN - 1) / BN);
  int m_tile, n_tile;
  tile_order(blockIdx.x, nb, mt, p.dMt, m_tile, n_tile);
  const int m0 = m_tile * BM, n0 = n_tile * BN;
  const int nch = (p.Cin + YKC - 1) / YKC;
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)p.wT, 0, (int)p.w_bytes, 0x00020000);
  // activation staging: this lane loads column n0 + xn, slices xkb0 .. xkb0 + XK - 1 of each chunk (the slice is wave-uniform)
  const int xn = lane + 64 * (wid % XG), xkb0 = __builtin_amdgcn_readfirstlane((wid / XG) * XK);
  const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc((void*)p.in, 0, (int)p.in_bytes, 0x00020000);
  unsigned xoff = OOB;
  {
    const int n = n0 + xn;
    if (n < p.Ntot) {
      const int img = fdiv(n, p.dNpix);
      xoff = (unsigned)(((size_t)img * p.Cin * p.Npix + (n - img * p.Npix)) * 4);
    }
  }
  const unsigned cstride = (unsigned)p.Npix * 4;     // bytes from one channel to the next
  float xr[2][XK * 8];
  u32x4 wr[2][WQ];
  auto gload = [&](auto set, int c) {
    constexpr int S = decltype(set)::value;
#pragma unroll
    for (int q = 0; q < XK; ++q) {
      const int k0 = c * YKC + 8 * (xkb0 + q);
      const unsigned base = k0 < p.Cin ? xoff : OOB;            // (the absent half of a K tail reads zeros, not the next image)
#pragma unroll
      for (int j = 0; j < 8; ++j) xr[S][q * 8 + j] = buf_ld1s(rin, base, (unsigned)(k0 + j) * cstride);
    }
#pragma unroll
    for (int q = 0; q < WQ; ++q) {
      const int e = tid + 256 * q, r = e % BM, kg = c * YKB + e / BM;                  // (kg >= Cin / 8: past the image, zeros)
      wr[S][q] = __builtin_bit_cast(u32x4, buf_ld4(rw, (unsigned)((kg * p.Mp + m0 + r) * 16)));
    }
  };
  auto lstore = [&](auto set) {                                  // chunk c of register set c & 1 into LDS stage c & 1
    constexpr int S = decltype(set)::value;
#pragma unroll
    for (int q = 0; q < WQ; ++q) As[S][tid + 256 * q] = wr[S][q];
#pragma unroll
    for (int q = 0; q < XK; ++q) Bs[S][(xkb0 + q) * BN + xn] = to_bf16x8(&xr[S][q * 8]);
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
  // C/D layout of the 32x32 MFMA: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  The epilogue is store_out's
  // arithmetic with its loads batched, as in k_conv1x1_bf16x3: per fragment the 16 scale / shift pairs and 16 residuals are all requested before
  // the first of them is used.
  int img[FN], rem[FN];
  bool col[FN];
#pragma unroll
  for (int j = 0; j < FN; ++j) {
    const int n = n0 + wn * (BN / 2) + j * 32 + (lane & 31);
    col[j] = n < p.Ntot;
    img[j] = col[j] ? fdiv(n, p.dNpix) : 0;
    rem[j] = n - img[j] * p.Npix;
  }
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
        rs[r] = (p.residual && col[j] && m < p.M) ? p.residual[((size_t)img[j] * p.M + m) * p.Npix + rem[j]] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = mb + (r & 3) + 8 * (r >> 2);
        float v = acc[i][j][r];
        if (p.scale) v = v * sc[r] + sh[r];
        if (p.residual) v += rs[r];
        if (p.relu) v = fmaxf(v, 0.f);
        if (col[j] && m < p.M) p.out[((size_t)img[j] * p.M + m) * p.Npix + rem[j]] = v;
      }
      __builtin_amdgcn_sched_barrier(0);          // one fragment's batch at a time
    }
}

std::atomic<long> g_bf16x1_launches{0};

int cu_count() {
  static const int N = [] {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess) (void)hipGetLastError();
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
    return cus;
  }();
  return N;
}

template <int BM, int BN, int YKC>
int launch_form(ConvParams p, hipStream_t st) {
  fill_divs(p, BM);
  const long nb = (long)((p.M + BM - 1) / BM) * ((p.Ntot + BN - 1) / BN);
  FRTM_CHECK_ARG(nb < 0x7fffffffL, "frtm_conv2d: too many tiles");
  k_conv1x1_bf16x1<BM, BN, YKC><<<(int)nb, 256, 0, st>>>(p);
  conv_trace("k_conv1x1_bf16x1<%d,%d,%d>", BM, BN, YKC);
  FRTM_LAUNCH_CHECK();
  g_bf16x1_launches += 1;
  return FRTM_OK;
}

}  // namespace

int frtm_bf16x1_pack(const float* src, int Cout, int Cin, int sm, int sk, float* out, hipStream_t st) {
  FRTM_CHECK_ARG(Cin % 16 == 0, "frtm_conv_pack_weights: the bf16x1 layout needs Cin %% 16 == 0 (got %d)", Cin);
  FRTM_CHECK_ARG(((size_t)out) % 16 == 0, "frtm_conv_pack_weights: the bf16x1 image must be 16-byte aligned");
  const int Mp = (Cout + YMP - 1) / YMP * YMP;
  const long total = (long)(Cin / 8) * Mp;
  k_pack_weights_bf16x1<<<(int)std::min<long>((total + 255) / 256, 2048), 256, 0, st>>>(src, Cout, Cin, sm, sk, Mp, (u32x4*)out);
  conv_trace("k_pack_weights_bf16x1");
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

// p as frtm_conv2d filled it for a 1x1 stride-1 conv; p.wT = the FRTM_WLAYOUT_BF16X1 image; tile: 0 = automatic, else FRTM_BF16X1_TILE_*
int frtm_bf16x1_launch(ConvParams p, int tile, hipStream_t st) {
  FRTM_CHECK_ARG(p.Cin % 16 == 0, "frtm_conv2d: the bf16x1 layout needs Cin %% 16 == 0 (got %d)", p.Cin);
  FRTM_CHECK_ARG(((size_t)p.wT) % 16 == 0, "frtm_conv2d: the bf16x1 image must be 16-byte aligned");
  FRTM_CHECK_ARG(tile >= 0 && tile <= FRTM_BF16X1_TILE_64x64, "frtm_conv2d: bf16x1 layout: tile selects the form (0 auto, 1 128x64, 2 64x64), got %d", tile);
  p.Mp = (p.M + YMP - 1) / YMP * YMP;
  p.w_bytes = (unsigned)((size_t)p.Cin * p.Mp * 2);             // (below the GEMM image's size, which frtm_conv2d checked against 2^31)
  p.splitk = 1;
  p.nchunks = p.chunks_per_split = (p.Cin + 63) / 64;
  if (tile == 0) {
    const long big = (long)((p.M + 127) / 128) * ((p.Ntot + 63) / 64);
    tile = (p.Cin >= 1024 && big >= cu_count()) ? FRTM_BF16X1_TILE_128x64 : FRTM_BF16X1_TILE_64x64;
  }
  return tile == FRTM_BF16X1_TILE_128x64 ? launch_form<128, 64, 64>(p, st) : launch_form<64, 64, 64>(p, st);
}

extern "C" long frtm_conv_bf16x1_launches(void) { return g_bf16x1_launches.load(); }
// a launch of this layout's format-aware form (csrc/conv_bf16act.hip) counts here as well
void frtm_bf16x1_count_launch() { g_bf16x1_launches += 1; }
