// bf16x1 weight gradient of a 3x3 convolution (opt-in refiner training mode, SegNetwork.train_precision = 'bf16x1'): stride 1, pad 1 (zeros),
// NCHW fp32 in, fp32 out, any B, Cin, Cout, H, W.
//
//   dW[co,ci,kh,kw] = sum_{n,y,x} bf16(dY[n,co,y,x]) * bf16(X[n,ci,y-1+kh,x-1+kw])     (zero outside the map)
//   dbias[co]       = sum_{n,y,x} bf16(dY[n,co,y,x])
//
// The arithmetic of conv3x3_bf16x1.hip: each operand is rounded to bf16 once, to nearest even (v_cvt_pk_bf16_f32, in registers on its way to LDS),
// the products run on v_mfma_f32_32x32x16_bf16, accumulation is fp32.  The two roundings cost up to 2^-7 of |dY| (x) |X| per element; this is NOT
// fp32-level arithmetic.  The bias is a ones column of the same product (1.0 is exact in bf16: only dY's rounding enters).
//
// The GEMM: M = Cout, N = (ci, tap), K = pixels.  A lane's eight k of an MFMA operand are eight consecutive pixels of one image row.  The pixels are
// cut into tiles of WT_H x WT_W = 4 rows x 32 columns of one image; a workgroup (four waves) owns 64 output channels x 32 input channels x 9 taps
// (+ the ones column in the workgroups of the first input-channel tile) and walks a contiguous range of tiles.  Per tile it stages
//   * dY's 64 x 4 x 32 values once, as bf16 [co][row][8-pixel unit],
//   * X's 32 x 6 x 34 halo patch as bf16 in THREE column-shifted copies [kw][ci][patch row][8-pixel unit]: copy kw holds the patch from column kw
//     on, so the operand of tap (kh, kw) is the 16-byte-aligned unit of copy kw at row + kh -- every read is one aligned ds_read_b128, the nine-fold
//     global gather of the fp32 kernel is gone (a thread loads ten consecutive floats -- as dwordx4 loads at dword alignment in a tile whose windows
//     all lie inside their rows, element by element in the tiles at the image's left and right edges -- and forms the three shifted units from them in registers).
//     Channel pitches of 25 and 17 units (odd): the 16 lanes of a ds_read_b128 group fall on 16 different 16-byte bank slots.
// Wave (wm, wk) multiplies output channels 32 wm .. + 31 with tile rows 2 wk, 2 wk + 1: nine 32 x 32 accumulators (co x ci, one per tap) and the
// ones column.  The global loads of tile t + 1 are requested into registers before the MFMAs of tile t; as compiled, the two load forms (below) join
// in one set of registers and the wait for them lands before those MFMAs, so a tile pays one exposed load latency.
// 468 registers per lane, no scratch: one workgroup per CU, which is what the plan's rounds of 256 workgroups assume.
//
// Zeros.  A position outside the image, a channel past Cin or Cout and a tile row or column past the image are loaded as zeros (buffer loads at an
// out-of-range offset), never as the neighbouring image's data.  A pixel slot past the image has dY = 0, but its shifted X can be a real value (the
// left neighbour of column W is column W - 1): a whole row or 16-pixel step past the image is skipped, and in a tile that overhangs the right edge
// the X operand's slots past column W - 1 are masked to zero, so a NaN or Inf in X reaches exactly the (ci, tap) columns that read it.
//
// Determinism.  No atomics.  Each wave's accumulators go to a slab of their own, part[2 split + wk][co][ci * 9 + tap | bias]; k_wgrad_bf16x1_reduce
// sums the slabs in fp64 in ascending order.  The plan (tiles per split) is a function of the shape alone, and the grid follows from it.  A wave's
// fp32 chain is its two rows of the split's tiles in ascending order: at most WT_MAX_TILES x 64 = 2048 pixels.
#include "conv_common.h"
#include "../../include/frtm_hip.h"
#include <atomic>
#include <type_traits>

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int WT_H = 4, WT_W = 32;            // pixel tile
constexpr int WT_CO = 64, WT_CI = 32;         // channel tile of a workgroup
constexpr int WT_MAX_TILES = 32;              // most tiles per split: bounds the fp32 chain
constexpr int WT_TARGET = 256;                // workgroups per round: one per CU (a workgroup's registers fill a CU's SIMDs)
constexpr int XCS = 25;                       // X: 16-byte units per channel (6 rows x 4 units = 24, + 1: odd)
constexpr int XKS = WT_CI * XCS;              // ... per column-shifted copy
constexpr int ACS = 17;                       // dY: units per channel (4 rows x 4 units = 16, + 1)
constexpr int XQ = WT_CI * 6 * 4 / 256;       // X items (channel, patch row, unit) per thread: 3
constexpr int AQ = WT_CO * 4 * 4 / 256;       // dY items per thread: 4

struct WgradParams {
  const float* dy; const float* x; float* part;
  int Cout, Cin, H, W, ncol, ntiles, tps, tpi, tx;      // tiles: in all, per split, per image, per tile row
  FastDiv dImg, dTx;                                     // divisions by tpi and tx
};

__global__ __launch_bounds__(256) void k_conv_wgrad_bf16x1(WgradParams p) {
  __shared__ __attribute__((aligned(16))) u32x4 Xs[3 * XKS], As[WT_CO * ACS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, h = lane >> 5;
  const int wm = wv >> 1, wk = wv & 1;
  const int split = blockIdx.x, ci0 = blockIdx.y * WT_CI, co0 = blockIdx.z * WT_CO;
  const bool bias_tile = blockIdx.y == 0;
  const int HW = p.H * p.W;
  const int t_lo = split * p.tps, t_hi = min(p.ntiles, t_lo + p.tps);
  const unsigned x_img = (unsigned)p.Cin * HW * 4, a_img = (unsigned)p.Cout * HW * 4;        // bytes of one image (the launcher checked < 2^31)

  // what this thread stages, tile after tile: X items tid + 256 q = (channel, patch row, unit), dY items = (channel, row, unit)
  int xr[XQ], xu[XQ], xdst[XQ], ar[AQ], au[AQ], adst[AQ];
  unsigned xch[XQ], ach[AQ];
#pragma unroll
  for (int q = 0; q < XQ; ++q) {
    const int it = tid + 256 * q, c = it / 24, rem = it - c * 24;
    xr[q] = rem >> 2; xu[q] = rem & 3;
    xdst[q] = c * XCS + rem;
    xch[q] = ci0 + c < p.Cin ? (unsigned)(ci0 + c) * HW * 4 : OOB;
  }
#pragma unroll
  for (int q = 0; q < AQ; ++q) {
    const int it = tid + 256 * q, c = it >> 4, rem = it & 15;
    ar[q] = rem >> 2; au[q] = rem & 3;
    adst[q] = c * ACS + rem;
    ach[q] = co0 + c < p.Cout ? (unsigned)(co0 + c) * HW * 4 : OOB;
  }
  float xv[XQ][10], av[AQ][8];
  auto gload = [&](int t, int& y0, int& x0) {
    const int img = fdiv(t, p.dImg), rem = t - img * p.tpi;
    const int tyi = fdiv(rem, p.dTx), txi = rem - tyi * p.tx;
    y0 = tyi * WT_H; x0 = txi * WT_W;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + (size_t)img * p.Cin * HW), 0, (int)x_img, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)(p.dy + (size_t)img * p.Cout * HW), 0, (int)a_img, 0x00020000);
    if (x0 >= 1 && x0 + WT_W + 1 < p.W) {
      // every window of the tile inside its row (wave-uniform): dwordx4 loads at dword alignment; a row outside the image or a channel past the
      // tensor's reads zeros through the offset
#pragma unroll
      for (int q = 0; q < XQ; ++q) {
        const int gy = y0 - 1 + xr[q], gx = x0 - 1 + 8 * xu[q];
        const unsigned off = (gy >= 0 && gy < p.H && xch[q] != OOB) ? xch[q] + (unsigned)(gy * p.W + gx) * 4 : OOB;
        const f32x4 v0 = buf_ld4s(rx, off, 0), v1 = buf_ld4s(rx, off, 16);
        xv[q][8] = buf_ld1s(rx, off, 32);
        xv[q][9] = buf_ld1s(rx, off, 36);
#pragma unroll
        for (int e = 0; e < 4; ++e) { xv[q][e] = v0[e]; xv[q][4 + e] = v1[e]; }
      }
#pragma unroll
      for (int q = 0; q < AQ; ++q) {
        const int gy = y0 + ar[q], gx = x0 + 8 * au[q];
        const unsigned off = (gy < p.H && ach[q] != OOB) ? ach[q] + (unsigned)(gy * p.W + gx) * 4 : OOB;
        const f32x4 v0 = buf_ld4s(ra, off, 0), v1 = buf_ld4s(ra, off, 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) { av[q][e] = v0[e]; av[q][4 + e] = v1[e]; }
      }
    } else {
      // a tile at the left or right edge of the image: element by element, a column outside the row reads zeros
#pragma unroll
      for (int q = 0; q < XQ; ++q) {
        const int gy = y0 - 1 + xr[q], gx = x0 - 1 + 8 * xu[q];
        const unsigned row = (gy >= 0 && gy < p.H) ? xch[q] : OOB;                       // OOB stays OOB: the channel offsets are below 2^31
        const unsigned base = row + (unsigned)(gy * p.W + gx) * 4;                       // (wraps where row is OOB or gx < 0: not used there)
#pragma unroll
        for (int e = 0; e < 10; ++e) xv[q][e] = buf_ld1(rx, (row != OOB && gx + e >= 0 && gx + e < p.W) ? base + 4 * e : OOB);
      }
#pragma unroll
      for (int q = 0; q < AQ; ++q) {
        const int gy = y0 + ar[q], gx = x0 + 8 * au[q];
        const unsigned row = gy < p.H ? ach[q] : OOB;
        const unsigned base = row + (unsigned)(gy * p.W + gx) * 4;
#pragma unroll
        for (int e = 0; e < 8; ++e) av[q][e] = buf_ld1(ra, (row != OOB && gx + e < p.W) ? base + 4 * e : OOB);
      }
    }
  };
  auto lstore = [&]() {
#pragma unroll
    for (int q = 0; q < XQ; ++q) {
      __bf16 hx[10];
#pragma unroll
      for (int e = 0; e < 10; ++e) hx[e] = (__bf16)xv[q][e];
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        bf16x8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = hx[kw + j];
        Xs[kw * XKS + xdst[q]] = __builtin_bit_cast(u32x4, v);
      }
    }
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
      bf16x8 v;
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (__bf16)av[q][j];
      As[adst[q]] = __builtin_bit_cast(u32x4, v);
    }
  };

  f32x16 acc[9], accb;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    accb[r] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t][r] = 0.f;
  }
  bf16x8 ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones[j] = (__bf16)1.0f;

  // one tile's products of this wave: rows 2 wk + j, 16-pixel steps s.  EDGE: the tile overhangs the right edge of the image
  const int abase = (wm * 32 + l31) * ACS + 2 * wk * 4 + h, bbase = l31 * XCS + 2 * wk * 4 + h;
  auto products = [&](int y0, int x0, auto edge) {
    constexpr bool EDGE = decltype(edge)::value;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (y0 + 2 * wk + j >= p.H) continue;                  // a row past the image: nothing to add (wave-uniform)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (EDGE && x0 + 16 * s >= p.W) continue;            // a step past the image (uniform)
        u32x4 mask;
        if (EDGE) {
          const int nv = p.W - x0 - 16 * s - 8 * h;          // pixels of this lane's unit inside the image
#pragma unroll
          for (int d = 0; d < 4; ++d) mask[d] = (nv > 2 * d ? 0x0000ffffu : 0u) | (nv > 2 * d + 1 ? 0xffff0000u : 0u);
        }
        const bf16x8 a = __builtin_bit_cast(bf16x8, As[abase + j * 4 + 2 * s]);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          const int kh = tap / 3, kw = tap - 3 * kh;
          u32x4 b = Xs[kw * XKS + bbase + (j + kh) * 4 + 2 * s];
          if (EDGE) b &= mask;
          acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, b), acc[tap], 0, 0, 0);
        }
        if (bias_tile) accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, ones, accb, 0, 0, 0);
      }
    }
  };

  int y0 = 0, x0 = 0, yn = 0, xn = 0;
  if (t_lo < t_hi) gload(t_lo, y0, x0);
  for (int t = t_lo; t < t_hi; ++t) {
    lstore();
    __syncthreads();
    if (t + 1 < t_hi) gload(t + 1, yn, xn);                  // the next tile's loads, requested before this tile's MFMAs
    if (x0 + WT_W > p.W) products(y0, x0, std::true_type());
    else products(y0, x0, std::false_type());
    __syncthreads();
    y0 = yn; x0 = xn;
  }

  // C/D layout of the 32x32 MFMA: column (ci) = lane & 31, row (co) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  float* slab = p.part + (size_t)(2 * split + wk) * p.Cout * p.ncol;
  const int ci = ci0 + l31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (co < p.Cout) {
      float* row = slab + (size_t)co * p.ncol;
      if (ci < p.Cin) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) row[ci * 9 + tap] = acc[tap][r];
      }
      if (bias_tile && l31 == 0) row[p.ncol - 1] = accb[r];
    }
  }
}

// fixed-order (fp64) sum of the slabs -> dW, dbias (the job of k_conv_wgrad_reduce of refiner_train.hip, which another translation unit cannot
// launch).  64 elements per workgroup, four threads per element: thread q adds the q-th quarter of the slabs in ascending order, eight loads in
// flight at a time, and the four partial sums are added in the order ((0 + 1) + 2) + 3: one fixed order for a given number of slabs.
__global__ __launch_bounds__(256) void k_wgrad_bf16x1_reduce(const float* __restrict__ part, int nslab, int Cout, int ncol, float* __restrict__ dw,
                                                              float* __restrict__ dbias) {
  __shared__ double red[4][64];
  const int e = threadIdx.x & 63, q = threadIdx.x >> 6, n = Cout * ncol;
  const int i = blockIdx.x * 64 + e;
  const int per = (nslab + 3) / 4, k0 = q * per, k1 = min(nslab, k0 + per);
  double s = 0.0;
  if (i < n) {
    const float* src = part + i;
    int k = k0;
    for (; k + 8 <= k1; k += 8) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = src[(size_t)(k + j) * n];
#pragma unroll
      for (int j = 0; j < 8; ++j) s += (double)v[j];
    }
    for (; k < k1; ++k) s += (double)src[(size_t)k * n];
  }
  red[q][e] = s;
  __syncthreads();
  if (q != 0 || i >= n) return;
  s = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
  const int co = i / ncol, j = i - co * ncol;
  if (j < ncol - 1) {
    if (dw) dw[(size_t)co * (ncol - 1) + j] = (float)s;
  } else if (dbias) {
    dbias[co] = (float)s;
  }
}

std::atomic<long> g_wgrad_bf16x1_launches{0};

// tiles of the launch, tiles per split, splits: the fewest rounds of WT_TARGET workgroups whose splits stay within WT_MAX_TILES tiles (the chain
// bound), and the splits that fill those rounds evenly.  false: too large
bool wgrad_plan(int B, int Cout, int Cin, int H, int W, WgradParams& p, int& nsplit) {
  const long long tx = (W + WT_W - 1) / WT_W, ty = (H + WT_H - 1) / WT_H, nt = (long long)B * ty * tx;
  if (nt >= 0x7fffffffLL || ty * tx >= 0x7fffffffLL) return false;
  const long long ct = (long long)((Cin + WT_CI - 1) / WT_CI) * ((Cout + WT_CO - 1) / WT_CO);
  const long long rounds = (nt * ct + (long long)WT_TARGET * WT_MAX_TILES - 1) / ((long long)WT_TARGET * WT_MAX_TILES);
  const long long tps = (nt * ct + WT_TARGET * rounds - 1) / (WT_TARGET * rounds);        // 1 .. WT_MAX_TILES
  p.ntiles = (int)nt; p.tps = (int)tps; p.tpi = (int)(ty * tx); p.tx = (int)tx;
  p.dImg = fast_div((unsigned)p.tpi); p.dTx = fast_div((unsigned)p.tx);
  nsplit = (int)((nt + tps - 1) / tps);
  return true;
}

}  // namespace

extern "C" size_t frtm_conv_wgrad_bf16x1_ws_elems(int B, int Cout, int Cin, int H, int W) {
  if (B <= 0 || Cout <= 0 || Cin <= 0 || H <= 0 || W <= 0) return 0;
  WgradParams p;
  int nsplit;
  if (!wgrad_plan(B, Cout, Cin, H, W, p, nsplit)) return 0;
  return (size_t)2 * nsplit * Cout * ((size_t)Cin * 9 + 1);
}

extern "C" int frtm_conv_wgrad_bf16x1(const float* dy, const float* x, int B, int Cout, int Cin, int H, int W, float* dw, float* dbias, float* ws,
                                      size_t ws_elems, frtm_stream_t stream) {
  FRTM_CHECK_ARG(dy && x && ws && (dw || dbias) && B > 0 && Cout > 0 && Cin > 0 && H > 0 && W > 0, "frtm_conv_wgrad_bf16x1: bad argument");
  FRTM_CHECK_ARG((size_t)H * W < 0x7fffffff && Cout <= 65535 * 64 && (long long)Cin * 9 < 0x7fffffff - 64, "frtm_conv_wgrad_bf16x1: too large");
  FRTM_CHECK_ARG((size_t)(Cout + WT_CO) * H * W * 4 < 0x7fffffffull && (size_t)(Cin + WT_CI) * H * W * 4 < 0x7fffffffull && Cin <= 65535 * WT_CI,
                 "frtm_conv_wgrad_bf16x1: an image too large for 32-bit buffer offsets");
  WgradParams p;
  int nsplit;
  FRTM_CHECK_ARG(wgrad_plan(B, Cout, Cin, H, W, p, nsplit), "frtm_conv_wgrad_bf16x1: too many pixel tiles");
  p.dy = dy; p.x = x; p.part = ws;
  p.Cout = Cout; p.Cin = Cin; p.H = H; p.W = W; p.ncol = Cin * 9 + 1;
  FRTM_CHECK_ARG((size_t)Cout * p.ncol < 0x7fffffff, "frtm_conv_wgrad_bf16x1: too large");
  const size_t need = (size_t)2 * nsplit * Cout * p.ncol;
  FRTM_CHECK_ARG(need <= ws_elems, "frtm_conv_wgrad_bf16x1: workspace of %zu floats, need %zu (frtm_conv_wgrad_bf16x1_ws_elems)", ws_elems, need);
  const dim3 g(nsplit, ceil_div(Cin, WT_CI), ceil_div(Cout, WT_CO));
  k_conv_wgrad_bf16x1<<<g, 256, 0, (hipStream_t)stream>>>(p);
  FRTM_LAUNCH_CHECK();
  k_wgrad_bf16x1_reduce<<<ceil_div(Cout * p.ncol, 64), 256, 0, (hipStream_t)stream>>>(ws, 2 * nsplit, Cout, p.ncol, dw, dbias);
  FRTM_LAUNCH_CHECK();
  g_wgrad_bf16x1_launches += 1;
  return FRTM_OK;
}

extern "C" long frtm_conv_wgrad_bf16x1_launches(void) { return g_wgrad_bf16x1_launches.load(); }
