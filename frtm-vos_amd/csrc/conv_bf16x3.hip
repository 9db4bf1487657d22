// bf16x3 1x1 convolution (opt-in trunk precision mode, FRTM_WLAYOUT_BF16X3): stride 1, pad 0, NCHW fp32 in and out, Cin % 16 == 0.
//
//   out[img, m, pix] = epilogue( sum_k W[m][k] X[img, k, pix] )     epilogue as frtm_conv2d: (* scale[m] + shift[m])?  (+ residual)?  relu?
//
// Both operands are split into three bf16 pieces, v = hi + mid + lo (hi = bf16(v), mid = bf16(v - hi), lo = bf16(v - hi - mid): the remainders are
// exact in fp32), and each product is formed from the six piece products of weight >= 2^-16 (hi.hi, hi.mid, mid.hi, hi.lo, mid.mid, lo.hi), in one
// fixed order per k-step of 16, smallest first:
//   W.lo X.hi, W.mid X.mid, W.hi X.lo, W.mid X.hi, W.hi X.mid, W.hi X.hi
// on v_mfma_f32_32x32x16_bf16 with fp32 accumulation (16x the fp32 MFMA rate: six products give a 2.67x higher ceiling).  The sum is NOT bitwise
// an fmaf chain: against an fp64 product, on the trunk's 1x1 shapes at 1 and 8 frames, max error 0.78-1.40x and rms error 0.93-1.28x those of the
// fp32 kernels (profiles/bf16x3_trunk_time.txt).  Largest first measured up to 1.73x the fp32 max error (64 -> 256 at 8 frames: the small
// products of a k-step then land on the running sum).  A NaN stays a NaN (the
// conversion is v_cvt_pk_bf16_f32, not integer rounding); an Inf input gives NaN (Inf - Inf in the split).  The result is deterministic: every
// output element is one workgroup's fixed sequence of MFMAs, whatever the grid.
//
// Weights are split once, at pack time, into three bf16 planes [3][Cin/8][Mp][8] (Mp = Cout rounded up to 128, zero padded): a lane's eight k of one
// MFMA operand are 16 contiguous bytes.  Activations are read from HBM as fp32, once, as the fp32 kernels read them, split in registers and staged in
// LDS in the same [piece][k/8][n][8] form: producers keep writing plain fp32.
//
// Tile 128 (Cout) x 128 (pixels of all images: tiles may straddle images, any H*W), four waves of 64 x 64 (2 x 2 fragments of 32 x 32), chunks of
// K = 16, two LDS stages (24 KB each): the global loads of chunk c + 1 are issued before the MFMAs of chunk c, and split and stored into the other
// stage after them; one barrier per chunk.  Split budget per chunk: 8 elements per lane at ~5.5 VALU each (1.5 cvt_pk, 2 subtractions, 2 widenings)
// = ~44 VALU beside 24 MFMAs of 32 cycles, i.e. fewer than 2 per MFMA gap (the gap hides ~5).  The next chunk's loads have only one chunk of MFMAs
// to land before its split waits on them.  220 VGPRs (the epilogue's batched loads): two waves per SIMD.
#include "conv_common.h"
#include "../../include/frtm_hip.h"
#include <atomic>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int XBM = 128, XBN = 128, XKC = 16;      // tile rows (Cout), columns (pixels), K per chunk

// v -> (hi, mid, lo), eight values at a time; each piece vector is the 16-byte MFMA operand of one lane
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const __bf16 hj = (__bf16)v[j];
    const float r1 = v[j] - (float)hj;
    const __bf16 mj = (__bf16)r1;
    const float r2 = r1 - (float)mj;
    h[j] = hj; m[j] = mj; l[j] = (__bf16)r2;
  }
}

// w(m, k) = src[m * sm + k * sk] (OIHW: sm = Cin, sk = 1; the backbone's packed GEMM image [Kp][Mp32]: sm = 1, sk = Mp32) -> P[3][Cin/8][Mp][8]
__global__ __launch_bounds__(256) void k_pack_weights_bf16x3(const float* __restrict__ src, int Cout, int Cin, int sm, int sk, int Mp, u32x4* __restrict__ P) {
  const int K8 = Cin / 8;
  const long total = (long)K8 * Mp;
  const size_t plane = (size_t)K8 * Mp;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const int m = (int)(e % Mp), kb = (int)(e / Mp);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = m < Cout ? src[(size_t)m * sm + (size_t)(kb * 8 + j) * sk] : 0.f;
    bf16x8 h, mid, l;
    split8(v, h, mid, l);
    P[e] = __builtin_bit_cast(u32x4, h);
    P[plane + e] = __builtin_bit_cast(u32x4, mid);
    P[2 * plane + e] = __builtin_bit_cast(u32x4, l);
  }
}

__global__ __launch_bounds__(256) void k_conv1x1_bf16x3(ConvParams p) {
  __shared__ __attribute__((aligned(16))) u32x4 As[2][3 * 2 * XBM], Bs[2][3 * 2 * XBN];     // [stage][piece][kb][row] x 16 bytes
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wm = wid >> 1, wn = wid & 1;
  const int mt = (p.M + XBM - 1) / XBM, nb = mt * ((p.Ntot + XBN - 1) / XBN);
  int m_tile, n_tile;
  tile_order(blockIdx.x, nb, mt, p.dMt, m_tile, n_tile);
  const int m0 = m_tile * XBM, n0 = n_tile * XBN;
  const int K8 = p.Cin / 8, nch = p.Cin / XKC;
  const u32x4* Wq = (const u32x4*)p.wT;
  // activation staging: this lane loads column n0 + xn, channels 8 xkb .. 8 xkb + 7 of each chunk (xkb is wave-uniform)
  const int xn = lane + 64 * (wid >> 1), xkb = __builtin_amdgcn_readfirstlane(wid & 1);
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
  float xr[8];
  u32x4 wr[3];
  auto gload = [&](int c) {
    const unsigned cb = (unsigned)(c * XKC + 8 * xkb) * cstride;
#pragma unroll
    for (int j = 0; j < 8; ++j) xr[j] = buf_ld1s(rin, xoff, cb + j * cstride);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int e = tid + 256 * q, r = e & (XBM - 1), kb = (e >> 7) & 1, pc = e >> 8;
      wr[q] = Wq[((size_t)pc * K8 + c * 2 + kb) * p.Mp + m0 + r];
    }
  };
  auto lstore = [&](int st) {
#pragma unroll
    for (int q = 0; q < 3; ++q) As[st][tid + 256 * q] = wr[q];
    bf16x8 h, m, l;
    split8(xr, h, m, l);
    Bs[st][(0 * 2 + xkb) * XBN + xn] = __builtin_bit_cast(u32x4, h);
    Bs[st][(1 * 2 + xkb) * XBN + xn] = __builtin_bit_cast(u32x4, m);
    Bs[st][(2 * 2 + xkb) * XBN + xn] = __builtin_bit_cast(u32x4, l);
  };
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  gload(0);
  lstore(0);
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    const int st = c & 1;
    if (c + 1 < nch) gload(c + 1);
    const int kb = lane >> 5;
    bf16x8 af[3][2], bf[3][2];
#pragma unroll
    for (int pc = 0; pc < 3; ++pc)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[pc][i] = __builtin_bit_cast(bf16x8, As[st][(pc * 2 + kb) * XBM + wm * 64 + i * 32 + (lane & 31)]);
        bf[pc][i] = __builtin_bit_cast(bf16x8, Bs[st][(pc * 2 + kb) * XBN + wn * 64 + i * 32 + (lane & 31)]);
      }
    // (weight piece, activation piece), smallest first: lo.hi, mid.mid, hi.lo, mid.hi, hi.mid, hi.hi
    constexpr int PA[6] = {2, 1, 0, 1, 0, 0}, PB[6] = {0, 1, 2, 0, 1, 0};
#pragma unroll
    for (int t = 0; t < 6; ++t)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[PA[t]][i], bf[PB[t]][j], acc[i][j], 0, 0, 0);
    if (c + 1 < nch) lstore(st ^ 1);
    __syncthreads();
  }
  // C/D layout of the 32x32 MFMA: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  The epilogue is store_out's
  // arithmetic with its loads batched: per 32 x 32 fragment the 16 scale / shift pairs and 16 residuals are all requested before the first of
  // them is used (one wait per batch instead of one per element).
  int img[2], rem[2];
  bool col[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + wn * 64 + j * 32 + (lane & 31);
    col[j] = n < p.Ntot;
    img[j] = col[j] ? fdiv(n, p.dNpix) : 0;
    rem[j] = n - img[j] * p.Npix;
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int mb = m0 + wm * 64 + i * 32 + 4 * (lane >> 5);
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
      __builtin_amdgcn_sched_barrier(0);          // one fragment's batch at a time: hoisting the next one's loads costs registers the K loop needs
    }
}

std::atomic<long> g_bf16x3_launches{0};

}  // namespace

int frtm_bf16x3_pack(const float* src, int Cout, int Cin, int sm, int sk, float* out, hipStream_t st) {
  FRTM_CHECK_ARG(Cin % 16 == 0, "frtm_conv_pack_weights: the bf16x3 layout needs Cin %% 16 == 0 (got %d)", Cin);
  FRTM_CHECK_ARG(((size_t)out) % 16 == 0, "frtm_conv_pack_weights: the bf16x3 image must be 16-byte aligned");
  const int Mp = (Cout + XBM - 1) / XBM * XBM;
  const long total = (long)(Cin / 8) * Mp;
  k_pack_weights_bf16x3<<<(int)std::min<long>((total + 255) / 256, 2048), 256, 0, st>>>(src, Cout, Cin, sm, sk, Mp, (u32x4*)out);
  conv_trace("k_pack_weights_bf16x3");
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

// p as frtm_conv2d filled it for a 1x1 stride-1 conv; p.wT = the FRTM_WLAYOUT_BF16X3 image
int frtm_bf16x3_launch(ConvParams p, hipStream_t st) {
  FRTM_CHECK_ARG(p.Cin % 16 == 0, "frtm_conv2d: the bf16x3 layout needs Cin %% 16 == 0 (got %d)", p.Cin);
  FRTM_CHECK_ARG(((size_t)p.wT) % 16 == 0, "frtm_conv2d: the bf16x3 image must be 16-byte aligned");
  p.Mp = (p.M + XBM - 1) / XBM * XBM;
  p.splitk = 1;
  p.nchunks = p.chunks_per_split = p.Cin / XKC;
  fill_divs(p, XBM);
  const long nb = (long)((p.M + XBM - 1) / XBM) * ((p.Ntot + XBN - 1) / XBN);
  FRTM_CHECK_ARG(nb < 0x7fffffffL, "frtm_conv2d: too many tiles");
  k_conv1x1_bf16x3<<<(int)nb, 256, 0, st>>>(p);
  conv_trace("k_conv1x1_bf16x3");
  FRTM_LAUNCH_CHECK();
  g_bf16x3_launches += 1;
  return FRTM_OK;
}

extern "C" long frtm_conv_bf16x3_launches(void) { return g_bf16x3_launches.load(); }
