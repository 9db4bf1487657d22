// Backward pass (and the train-mode BatchNorm) of the refinement network (model/seg_network.py), for
// SegNetwork.forward_train (model/refiner_train.py).  The forward reuses the inference kernels (frtm_conv2d, refiner_ops.hip);
// the input gradient of every convolution is a forward frtm_conv2d on flipped / transposed weights.  What is new here:
//   k_conv_wgrad          dW = dY (x) X over all pixels: fp32 MFMA, split over pixels into partial slabs
//   k_conv_wgrad_reduce   fixed-order (fp64) sum of the slabs -> dW, dbias
//   k_bn_*                train-mode BatchNorm statistics, apply + ReLU, backward (masked by the ReLU)
//   k_relu_bwd            dy * (y > 0)
//   k_pyrup2x_bwd_axis    transpose of k_pyrup2x along one axis (gather)
//   k_bilinear_bwd_axis   transpose of k_bilinear_resize along one axis (gather)
//   k_cab_*               channel-attention combine and gate backward
//   k_shift9              the nine zero-filled shifts of the logit gradient (head tail: conv2's taps before the resampling)
// No kernel here uses atomics: every sum runs in a fixed order, so two identical backward passes give bit-identical gradients.
#include "frtm_common.h"
#include "resample_taps.h"
#include "../../include/frtm_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------
// Weight gradient of a stride-1 conv with a k x k kernel (k = 1 or 3), pad k/2:
//   dW[co, ci*T + t] = sum_{n,y,x} dY[n,co,y,x] * X[n,ci,y+dy_t,x+dx_t]   (zero outside),  T = k*k
// A GEMM with M = Cout, N = Cin*T + 1 (the last column reads 1: dbias = sum dY) and K = B*H*W pixels.  A workgroup
// computes a 64 x 64 tile of (co, column) over one chunk of pixels with v_mfma_f32_32x32x2_f32 (2 x 2 waves of 32 x 32) and
// writes it to its slab part[split][co][column]; k_conv_wgrad_reduce sums the slabs.  Inside a chunk the MFMA chain runs over
// WG_SUB pixels and is then added into a second accumulator, so no fp32 chain is longer than WG_SUB (+ chunk / WG_SUB) terms.
// ------------------------------------------------------------------------------------------
#define WG_KB 32          // pixels per LDS stage
#define WG_SUB 128        // pixels per MFMA chain
#define WG_LD 33          // LDS row pitch (floats): [row][pixel]

template <int T>
__global__ __launch_bounds__(256) void k_conv_wgrad(const float* __restrict__ dy, const float* __restrict__ x, int Cout, int Cin, int H, int W,
                                                     int ncol, long long K, int kchunk, float* __restrict__ part) {
  __shared__ float As[64 * WG_LD];                           // [co][pixel]
  __shared__ float Bs[64 * WG_LD];                           // [column][pixel]
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  const int col0 = blockIdx.x * 64, co0 = blockIdx.y * 64, split = blockIdx.z;
  const long long k_lo = (long long)split * kchunk, k_hi = min(K, k_lo + kchunk);
  const int HW = H * W;
  const int px = tid & 31, r0 = tid >> 5;                    // loader: pixel px of the stage, rows r0 + 8q
  f32x16 acc, tot;
#pragma unroll
  for (int i = 0; i < 16; ++i) { acc[i] = 0.f; tot[i] = 0.f; }
  float va[8], vb[8];
  auto load = [&](long long kb) {
    const long long P = kb + px;
    const bool ok = P < k_hi;
    int n = 0, rem = 0, yy = 0, xx = 0;
    if (ok) { n = (int)(P / HW); rem = (int)(P - (long long)n * HW); yy = rem / W; xx = rem - yy * W; }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int co = co0 + r0 + 8 * q;
      va[q] = (ok && co < Cout) ? dy[((size_t)n * Cout + co) * HW + rem] : 0.f;
      const int j = col0 + r0 + 8 * q;
      float v = 0.f;
      if (ok && j < ncol - 1) {
        const int ci = j / T, t = j - ci * T;
        const int sy = yy + (T == 9 ? t / 3 - 1 : 0), sx = xx + (T == 9 ? t % 3 - 1 : 0);
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) v = x[((size_t)n * Cin + ci) * HW + sy * W + sx];
      } else if (ok && j == ncol - 1) {
        v = 1.f;
      }
      vb[q] = v;
    }
  };
  load(k_lo);
  int sub = 0;
  for (long long kb = k_lo; kb < k_hi; kb += WG_KB) {
#pragma unroll
    for (int q = 0; q < 8; ++q) { As[(r0 + 8 * q) * WG_LD + px] = va[q]; Bs[(r0 + 8 * q) * WG_LD + px] = vb[q]; }
    __syncthreads();
    if (kb + WG_KB < k_hi) load(kb + WG_KB);               // next stage's loads in flight during the MFMAs
    const float* a = As + (wm * 32 + (lane & 31)) * WG_LD + (lane >> 5);
    const float* b = Bs + (wn * 32 + (lane & 31)) * WG_LD + (lane >> 5);
#pragma unroll
    for (int kk = 0; kk < WG_KB; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kk], b[kk], acc, 0, 0, 0);
    __syncthreads();
    sub += WG_KB;
    if (sub == WG_SUB) {
      sub = 0;
#pragma unroll
      for (int i = 0; i < 16; ++i) { tot[i] += acc[i]; acc[i] = 0.f; }
    }
  }
  // C/D map of 32x32 f32: column = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  const int j = col0 + wn * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (co < Cout && j < ncol) part[((size_t)split * Cout + co) * ncol + j] = tot[r] + acc[r];
  }
}

__global__ __launch_bounds__(256) void k_conv_wgrad_reduce(const float* __restrict__ part, int nsplit, int Cout, int ncol, float* __restrict__ dw,
                                                            float* __restrict__ dbias) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Cout * ncol) return;
  double s = 0.0;
  for (int k = 0; k < nsplit; ++k) s += (double)part[(size_t)k * Cout * ncol + i];
  const int co = i / ncol, j = i - co * ncol;
  if (j < ncol - 1) {
    if (dw) dw[(size_t)co * (ncol - 1) + j] = (float)s;
  } else if (dbias) {
    dbias[co] = (float)s;
  }
}

static void wgrad_plan(int Cout, int ncol, long long K, int& nsplit, int& kchunk) {
  const int tiles = ceil_div(ncol, 64) * ceil_div(Cout, 64);
  const long long most = (K + WG_SUB - 1) / WG_SUB;            // at least one full chain per split
  long long s = 2048 / tiles;
  s = s < 1 ? 1 : s;
  s = s > most ? most : s;
  long long c = (K + s - 1) / s;
  c = (c + WG_KB - 1) / WG_KB * WG_KB;
  kchunk = (int)c;
  nsplit = (int)((K + c - 1) / c);
}

// ------------------------------------------------------------------------------------------
// BatchNorm (train mode: batch statistics; eval mode: running statistics) followed by ReLU
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void block_sum2_d(double& a, double& b, double* red) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_xor(a, off, 64); b += __shfl_xor(b, off, 64); }
  __syncthreads();
  if (lane == 0) { red[wid] = a; red[16 + wid] = b; }
  __syncthreads();
  double ta = 0.0, tb = 0.0;
  for (int i = 0; i < nw; ++i) { ta += red[i]; tb += red[16 + i]; }
  a = ta; b = tb;
}

// part[(c * N + n) * 2 + {0, 1}] = sum, sum of squares of plane (n, c); one block per plane
__global__ __launch_bounds__(256) void k_bn_stats_part(const float* __restrict__ x, int C, int HW, double* __restrict__ part) {
  __shared__ double red[32];
  const int n = blockIdx.x, c = blockIdx.y, N = gridDim.x;
  const float* p = x + ((size_t)n * C + c) * HW;
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < HW; i += 256) { const double v = p[i]; s += v; q += v * v; }
  block_sum2_d(s, q, red);
  if (threadIdx.x == 0) { part[((size_t)c * N + n) * 2] = s; part[((size_t)c * N + n) * 2 + 1] = q; }
}

// per channel: mean and 1/sqrt(var + eps) used for normalising (biased variance over N*HW), and in train mode the running-statistics
// update of nn.BatchNorm2d: r = (1 - f) r + f stat, with the unbiased variance.  train = 0: mean / invstd from the running statistics.
__global__ __launch_bounds__(256) void k_bn_stats_final(const double* __restrict__ part, int N, int C, int HW, float eps, float factor, int train,
                                                         float* __restrict__ rmean, float* __restrict__ rvar, float* __restrict__ mean,
                                                         float* __restrict__ invstd) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  if (!train) {
    mean[c] = rmean[c];
    invstd[c] = (float)(1.0 / sqrt((double)rvar[c] + (double)eps));
    return;
  }
  double s = 0.0, q = 0.0;
  for (int n = 0; n < N; ++n) { s += part[((size_t)c * N + n) * 2]; q += part[((size_t)c * N + n) * 2 + 1]; }
  const double cnt = (double)N * HW, m = s / cnt;
  double var = q / cnt - m * m;
  var = var < 0.0 ? 0.0 : var;
  mean[c] = (float)m;
  invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
  if (rmean && factor != 0.f) {
    const double f = factor;
    rmean[c] = (float)((1.0 - f) * rmean[c] + f * m);
    rvar[c] = (float)((1.0 - f) * rvar[c] + f * (cnt > 1.0 ? var * cnt / (cnt - 1.0) : var));
  }
}

// out = relu((x - mean) * invstd * gamma + beta); grid (ceil(HW / 256), N * C)
__global__ __launch_bounds__(256) void k_bn_apply_relu(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ invstd,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta, int C, int HW,
                                                        float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x, pl = blockIdx.y, c = pl % C;
  if (i >= HW) return;
  const float a = invstd[c] * gamma[c];
  const size_t o = (size_t)pl * HW + i;
  out[o] = fmaxf((x[o] - mean[c]) * a + beta[c], 0.f);
}

// backward, pass 1: g = dy * (out > 0); part[(c * N + n) * 3 + {0, 1, 2}] = sum g, sum g * xhat, sum xhat over plane (n, c).  The third sum is not
// zero: xhat is centred on the fp32 mean, which lies up to half an ulp from the mean of x
__global__ __launch_bounds__(256) void k_bn_bwd_part(const float* __restrict__ dy, const float* __restrict__ out, const float* __restrict__ x,
                                                      const float* __restrict__ mean, const float* __restrict__ invstd, int C, int HW,
                                                      double* __restrict__ part) {
  __shared__ double red[32];
  const int n = blockIdx.x, c = blockIdx.y, N = gridDim.x;
  const size_t o = ((size_t)n * C + c) * HW;
  const float m = mean[c], is = invstd[c];
  double s = 0.0, q = 0.0, xs = 0.0, none = 0.0;
  for (int i = threadIdx.x; i < HW; i += 256) {
    const float g = out[o + i] > 0.f ? dy[o + i] : 0.f;
    s += g;
    q += (double)g * (double)((x[o + i] - m) * is);
    xs += ((double)x[o + i] - (double)m) * (double)is;         // as k_bn_bwd_apply forms xhat
  }
  block_sum2_d(s, q, red);
  block_sum2_d(xs, none, red);
  if (threadIdx.x == 0) {
    part[((size_t)c * N + n) * 3] = s;
    part[((size_t)c * N + n) * 3 + 1] = q;
    part[((size_t)c * N + n) * 3 + 2] = xs;
  }
}

// backward, pass 2: every block sums its channel's partials in the same fixed order, then
//   train: dx = gamma * invstd / cnt * (cnt * g - sum g - (xhat - sum xhat / cnt) * sum g xhat)      eval: dx = gamma * invstd * g
// and the first block of each channel writes dgamma = sum g xhat, dbeta = sum g.  grid (ceil(HW / 256), N * C)
__global__ __launch_bounds__(256) void k_bn_bwd_apply(const float* __restrict__ dy, const float* __restrict__ out, const float* __restrict__ x,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma, const double* __restrict__ part, int N, int C, int HW,
                                                       int train, float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int i = blockIdx.x * 256 + threadIdx.x, pl = blockIdx.y, c = pl % C;
  double s = 0.0, q = 0.0, xs = 0.0;
  for (int n = 0; n < N; ++n) {
    s += part[((size_t)c * N + n) * 3];
    q += part[((size_t)c * N + n) * 3 + 1];
    xs += part[((size_t)c * N + n) * 3 + 2];
  }
  if (blockIdx.x == 0 && pl == c && threadIdx.x == 0) {
    if (dgamma) dgamma[c] = (float)q;
    if (dbeta) dbeta[c] = (float)s;
  }
  if (i >= HW) return;
  const size_t o = (size_t)pl * HW + i;
  const float g = out[o] > 0.f ? dy[o] : 0.f;
  const float is = invstd[c], a = gamma[c] * is;
  if (train) {
    const double cnt = (double)N * HW;
    // in fp64 with one final rounding: fp32 copies of sum g / n and sum g xhat / n would put the same rounding into every element of the
    // channel, and the conv bias in front, whose gradient is sum dx = 0 exactly, would collect it n times.  For the same reason xhat is
    // re-centred by its own mean in the last term: the fp32 mean alone leaves sum dx = -gamma invstd^2 (sum g xhat) (mean of x - mean[c])
    const double xh = ((double)x[o] - (double)mean[c]) * (double)is;
    dx[o] = (float)((double)gamma[c] * (double)is * ((double)g - s / cnt - (xh - xs / cnt) * (q / cnt)));
  } else {
    dx[o] = a * g;
  }
}

// dx = y > 0 ? dy : 0  (the gradient of ReLU, taken from the saved post-ReLU output; 0 at 0 like LeakyReLU(0))
__global__ __launch_bounds__(256) void k_relu_bwd(const float* __restrict__ dy, const float* __restrict__ y, size_t n, float* __restrict__ dx) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) dx[i] = y[i] > 0.f ? dy[i] : 0.f;
}

// ------------------------------------------------------------------------------------------
// Resampling transposes.  Both resamplings are separable; each backward kernel transposes one axis of a tensor viewed as
// (outer, L, inner): in (outer, Lout, inner) -> out (outer, Lin, inner), one thread per output element gathering the outputs of
// the forward that read it.  Rows and columns are two launches.
// ------------------------------------------------------------------------------------------
// weight of input i (of n) in output q of k_pyrup2x along one axis: output 2a reads in[a-2 .. a+1] with (E3,E2,E1,E0), output
// 2a+1 reads in[a-1 .. a+2] with (E0,E1,E2,E3), indices clamped into the map (replicate border)
__device__ __forceinline__ float pyr_w(int q, int i, int n) {
  const float E[4] = {PYR2X_E0, PYR2X_E1, PYR2X_E2, PYR2X_E3};
  const int a = q >> 1, odd = q & 1;
  float w = 0.f;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int src = min(max(a + m - 2 + odd, 0), n - 1);
    if (src == i) w += odd ? E[m] : E[3 - m];
  }
  return w;
}

__global__ __launch_bounds__(256) void k_pyrup2x_bwd_axis(const float* __restrict__ in, int n, int inner, size_t total, float* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int b = (int)(e % inner);
  const int i = (int)((e / inner) % n);
  const size_t o = e / ((size_t)inner * n);
  const float* p = in + o * (size_t)(2 * n) * inner + b;
  const int q0 = max(0, 2 * i - 3), q1 = min(2 * n - 1, 2 * i + 4);   // every output that reads input i, borders included
  float s = 0.f;
  for (int q = q0; q <= q1; ++q) s += pyr_w(q, i, n) * p[(size_t)q * inner];
  out[e] = s;
}

// in: (outer, Lout, inner) gradient of the resized map, out: (outer, Lin, inner).  The outputs that read input i form one range (the
// taps are monotone in the output index): [first d with i1(d) >= i, last d with i0(d) <= i], found by bisection.
__global__ __launch_bounds__(256) void k_bilinear_bwd_axis(const float* __restrict__ in, int Lin, int Lout, int inner, size_t total,
                                                            float* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int b = (int)(e % inner);
  const int i = (int)((e / inner) % Lin);
  const size_t o = e / ((size_t)inner * Lin);
  const float scale = (float)Lin / (float)Lout;
  int i0, i1; float l0, l1;
  int lo = 0, hi = Lout;                                      // first d with i1(d) >= i
  while (lo < hi) { const int m = (lo + hi) >> 1; bilinear_taps(m, scale, Lin, i0, i1, l0, l1); if (i1 >= i) hi = m; else lo = m + 1; }
  const int d0 = lo;
  lo = 0; hi = Lout;                                          // first d with i0(d) > i
  while (lo < hi) { const int m = (lo + hi) >> 1; bilinear_taps(m, scale, Lin, i0, i1, l0, l1); if (i0 > i) hi = m; else lo = m + 1; }
  const int d1 = lo;
  const float* p = in + o * (size_t)Lout * inner + b;
  float s = 0.f;
  for (int d = d0; d < d1; ++d) {
    bilinear_taps(d, scale, Lin, i0, i1, l0, l1);
    const float w = (i0 == i ? l0 : 0.f) + (i1 == i ? l1 : 0.f);
    s += w * p[(size_t)d * inner];
  }
  out[e] = s;
}

// ------------------------------------------------------------------------------------------
// CAB (seg_network.py: out = s * sigmoid(g) + up(d), g = conv(relu(conv([pool(s), pool(d)]))))
// ------------------------------------------------------------------------------------------
// per plane: a = sum dout * s, b = sum dout; one block per plane
__global__ __launch_bounds__(256) void k_cab_bwd_reduce(const float* __restrict__ dout, const float* __restrict__ s, int HW, float* __restrict__ a,
                                                         float* __restrict__ b) {
  __shared__ double red[32];
  const size_t o = (size_t)blockIdx.x * HW;
  double x = 0.0, y = 0.0;
  for (int i = threadIdx.x; i < HW; i += 256) { const float g = dout[o + i]; x += (double)g * s[o + i]; y += g; }
  block_sum2_d(x, y, red);
  if (threadIdx.x == 0) { a[blockIdx.x] = (float)x; b[blockIdx.x] = (float)y; }
}

// Gate backward, one block: v = [sp; dp] (n, 2oc), hid = relu(W1 v + b1), g = W2 hid + b2, dg = a * sig'(g).  W1 (oc, 2oc), W2 (oc, oc)
// in the conv layout [out][in].  Writes dW1, db1, dW2, db2 (each may be NULL), dsp (n, oc) and ddp (n, oc) (+ badd when given: the
// gradient of the broadcast term of the deepest CAB, whose deeper input is the pooled vector itself).  All sums over samples in order.
__global__ __launch_bounds__(256) void k_cab_gate_bwd(const float* __restrict__ sp, const float* __restrict__ dp, const float* __restrict__ gate,
                                                       const float* __restrict__ a, const float* __restrict__ badd, const float* __restrict__ W1,
                                                       const float* __restrict__ b1, const float* __restrict__ W2, int n, int oc,
                                                       float* __restrict__ dW1, float* __restrict__ db1, float* __restrict__ dW2,
                                                       float* __restrict__ db2, float* __restrict__ dsp, float* __restrict__ ddp) {
  extern __shared__ float sm[];
  float* v = sm;                      // n x 2oc
  float* hid = v + n * 2 * oc;        // n x oc
  float* dg = hid + n * oc;           // n x oc
  float* dh = dg + n * oc;            // n x oc
  const int tid = threadIdx.x, oc2 = 2 * oc;
  for (int e = tid; e < n * oc2; e += 256) {
    const int s = e / oc2, i = e - s * oc2;
    v[e] = i < oc ? sp[s * oc + i] : dp[s * oc + i - oc];
  }
  __syncthreads();
  for (int e = tid; e < n * oc; e += 256) {
    const int s = e / oc, j = e - s * oc;
    float acc = b1[j];
    for (int i = 0; i < oc2; ++i) acc += W1[j * oc2 + i] * v[s * oc2 + i];
    hid[e] = fmaxf(acc, 0.f);
    const float sg = 1.f / (1.f + __expf(-gate[e]));
    dg[e] = a[e] * sg * (1.f - sg);
  }
  __syncthreads();
  for (int e = tid; e < oc * oc; e += 256) {                  // dW2[k][j] = sum_s dg[s][k] hid[s][j]
    const int k = e / oc, j = e - k * oc;
    float acc = 0.f;
    for (int s = 0; s < n; ++s) acc += dg[s * oc + k] * hid[s * oc + j];
    if (dW2) dW2[e] = acc;
  }
  for (int k = tid; k < oc; k += 256) {
    float acc = 0.f;
    for (int s = 0; s < n; ++s) acc += dg[s * oc + k];
    if (db2) db2[k] = acc;
  }
  for (int e = tid; e < n * oc; e += 256) {                   // dh[s][j] = (hid > 0) sum_k W2[k][j] dg[s][k]
    const int s = e / oc, j = e - s * oc;
    float acc = 0.f;
    for (int k = 0; k < oc; ++k) acc += W2[k * oc + j] * dg[s * oc + k];
    dh[e] = hid[e] > 0.f ? acc : 0.f;
  }
  __syncthreads();
  for (int e = tid; e < oc * oc2; e += 256) {                 // dW1[j][i] = sum_s dh[s][j] v[s][i]
    const int j = e / oc2, i = e - j * oc2;
    float acc = 0.f;
    for (int s = 0; s < n; ++s) acc += dh[s * oc + j] * v[s * oc2 + i];
    if (dW1) dW1[e] = acc;
  }
  for (int j = tid; j < oc; j += 256) {
    float acc = 0.f;
    for (int s = 0; s < n; ++s) acc += dh[s * oc + j];
    if (db1) db1[j] = acc;
  }
  for (int e = tid; e < n * oc2; e += 256) {                  // dv[s][i] = sum_j W1[j][i] dh[s][j]
    const int s = e / oc2, i = e - s * oc2;
    float acc = 0.f;
    for (int j = 0; j < oc; ++j) acc += W1[j * oc2 + i] * dh[s * oc + j];
    if (i < oc) dsp[s * oc + i] = acc;
    else ddp[s * oc + i - oc] = acc + (badd ? badd[s * oc + i - oc] : 0.f);
  }
}

// ds = dout * sigmoid(gate) + dsp / HW  (the direct term and the pooled term); grid (ceil(HW / 256), planes)
__global__ __launch_bounds__(256) void k_cab_bwd_shallow(const float* __restrict__ dout, const float* __restrict__ gate, const float* __restrict__ dsp,
                                                          int HW, float* __restrict__ ds) {
  const int i = blockIdx.x * 256 + threadIdx.x, pl = blockIdx.y;
  if (i >= HW) return;
  const float sg = 1.f / (1.f + __expf(-gate[pl]));
  const size_t o = (size_t)pl * HW + i;
  ds[o] = dout[o] * sg + dsp[pl] / (float)HW;
}

// x[plane] += v[plane / group] * scale (the gradient of a plane mean broadcast back); grid (ceil(HW / 256), planes)
__global__ __launch_bounds__(256) void k_add_plane(float* __restrict__ x, const float* __restrict__ v, float scale, int HW) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= HW) return;
  x[(size_t)blockIdx.y * HW + i] += v[blockIdx.y] * scale;
}

// Head tail: out[n, t] = dl[n] shifted by tap t = (ky, kx): out[n,t,y,x] = dl[n, y - ky + 1, x - kx + 1] (0 outside)
__global__ __launch_bounds__(256) void k_shift9(const float* __restrict__ dl, int H, int W, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (i >= H * W) return;
  const int y = i / W, x = i - y * W;
  const float* p = dl + (size_t)n * H * W;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int sy = y - t / 3 + 1, sx = x - t % 3 + 1;
    out[((size_t)n * 9 + t) * H * W + i] = (sy >= 0 && sy < H && sx >= 0 && sx < W) ? p[sy * W + sx] : 0.f;
  }
}

extern "C" {

size_t frtm_conv_wgrad_ws_elems(int B, int Cout, int Cin, int k, int H, int W) {
  if (B <= 0 || Cout <= 0 || Cin <= 0 || H <= 0 || W <= 0 || (k != 1 && k != 3)) return 0;
  int nsplit, kchunk;
  const int ncol = Cin * k * k + 1;
  wgrad_plan(Cout, ncol, (long long)B * H * W, nsplit, kchunk);
  return (size_t)nsplit * Cout * ncol;
}

int frtm_conv_wgrad(const float* dy, const float* x, int B, int Cout, int Cin, int k, int H, int W, float* dw, float* dbias, float* ws,
                    size_t ws_elems, frtm_stream_t stream) {
  FRTM_CHECK_ARG(dy && x && ws && (dw || dbias) && B > 0 && Cout > 0 && Cin > 0 && H > 0 && W > 0, "frtm_conv_wgrad: bad argument");
  FRTM_CHECK_ARG(k == 1 || k == 3, "frtm_conv_wgrad: kernel size must be 1 or 3 (got %d)", k);
  FRTM_CHECK_ARG((size_t)H * W < 0x7fffffff && Cout <= 65535 * 64 && (long long)Cin * k * k < 0x7fffffff - 64, "frtm_conv_wgrad: too large");
  const int ncol = Cin * k * k + 1;
  int nsplit, kchunk;
  wgrad_plan(Cout, ncol, (long long)B * H * W, nsplit, kchunk);
  FRTM_CHECK_ARG((size_t)nsplit * Cout * ncol <= ws_elems, "frtm_conv_wgrad: workspace of %zu floats, need %zu (frtm_conv_wgrad_ws_elems)",
                 ws_elems, (size_t)nsplit * Cout * ncol);
  dim3 g(ceil_div(ncol, 64), ceil_div(Cout, 64), nsplit);
  if (k == 1)
    k_conv_wgrad<1><<<g, 256, 0, (hipStream_t)stream>>>(dy, x, Cout, Cin, H, W, ncol, (long long)B * H * W, kchunk, ws);
  else
    k_conv_wgrad<9><<<g, 256, 0, (hipStream_t)stream>>>(dy, x, Cout, Cin, H, W, ncol, (long long)B * H * W, kchunk, ws);
  FRTM_LAUNCH_CHECK();
  k_conv_wgrad_reduce<<<ceil_div(Cout * ncol, 256), 256, 0, (hipStream_t)stream>>>(ws, nsplit, Cout, ncol, dw, dbias);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_bn_stats(const float* x, int N, int C, int HW, float eps, float factor, int train, float* rmean, float* rvar, float* mean,
                  float* invstd, double* part, frtm_stream_t stream) {
  FRTM_CHECK_ARG(x && mean && invstd && N > 0 && C > 0 && HW > 0 && N <= 65535 && C <= 65535, "frtm_bn_stats: bad argument");
  FRTM_CHECK_ARG(train ? (part != nullptr && ((rmean == nullptr) == (rvar == nullptr))) : (rmean && rvar), "frtm_bn_stats: missing buffers");
  if (train) {
    k_bn_stats_part<<<dim3(N, C), 256, 0, (hipStream_t)stream>>>(x, C, HW, part);
    FRTM_LAUNCH_CHECK();
  }
  k_bn_stats_final<<<ceil_div(C, 256), 256, 0, (hipStream_t)stream>>>(part, N, C, HW, eps, factor, train, rmean, rvar, mean, invstd);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_bn_apply_relu(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta, int N, int C, int HW,
                       float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(x && mean && invstd && gamma && beta && out && N > 0 && C > 0 && HW > 0 && (size_t)N * C <= 65535,
                 "frtm_bn_apply_relu: bad argument");
  k_bn_apply_relu<<<dim3(ceil_div(HW, 256), N * C), 256, 0, (hipStream_t)stream>>>(x, mean, invstd, gamma, beta, C, HW, out);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_bn_relu_backward(const float* dy, const float* out, const float* x, const float* mean, const float* invstd, const float* gamma,
                          int N, int C, int HW, int train, float* dx, float* dgamma, float* dbeta, double* part, frtm_stream_t stream) {
  FRTM_CHECK_ARG(dy && out && x && mean && invstd && gamma && dx && part && N > 0 && C > 0 && HW > 0 && (size_t)N * C <= 65535,
                 "frtm_bn_relu_backward: bad argument");
  k_bn_bwd_part<<<dim3(N, C), 256, 0, (hipStream_t)stream>>>(dy, out, x, mean, invstd, C, HW, part);
  FRTM_LAUNCH_CHECK();
  k_bn_bwd_apply<<<dim3(ceil_div(HW, 256), N * C), 256, 0, (hipStream_t)stream>>>(dy, out, x, mean, invstd, gamma, part, N, C, HW, train, dx,
                                                                                   dgamma, dbeta);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_relu_backward(const float* dy, const float* y, size_t n, float* dx, frtm_stream_t stream) {
  FRTM_CHECK_ARG(dy && y && dx && n > 0, "frtm_relu_backward: bad argument");
  k_relu_bwd<<<(int)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384), 256, 0, (hipStream_t)stream>>>(dy, y, n, dx);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_pyrup2x_backward(const float* dout, int planes, int h, int w, float* din, float* tmp, frtm_stream_t stream) {
  FRTM_CHECK_ARG(dout && din && tmp && planes > 0 && h > 0 && w > 0, "frtm_pyrup2x_backward: bad argument");
  size_t t1 = (size_t)planes * 2 * h * w;                   // columns: (planes * 2h, 2w) -> (planes * 2h, w)
  FRTM_CHECK_ARG((t1 + 255) / 256 < 0x7fffffff, "frtm_pyrup2x_backward: too large");
  k_pyrup2x_bwd_axis<<<(unsigned)((t1 + 255) / 256), 256, 0, (hipStream_t)stream>>>(dout, w, 1, t1, tmp);
  FRTM_LAUNCH_CHECK();
  size_t t2 = (size_t)planes * h * w;                       // rows: (planes, 2h, w) -> (planes, h, w)
  k_pyrup2x_bwd_axis<<<(unsigned)((t2 + 255) / 256), 256, 0, (hipStream_t)stream>>>(tmp, h, w, t2, din);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_bilinear_backward(const float* dout, int planes, int h, int w, int H, int W, float* din, float* tmp, frtm_stream_t stream) {
  FRTM_CHECK_ARG(dout && din && tmp && planes > 0 && h > 0 && w > 0 && H > 0 && W > 0, "frtm_bilinear_backward: bad argument");
  size_t t1 = (size_t)planes * H * w;                       // columns: (planes * H, W) -> (planes * H, w)
  FRTM_CHECK_ARG((t1 + 255) / 256 < 0x7fffffff, "frtm_bilinear_backward: too large");
  k_bilinear_bwd_axis<<<(unsigned)((t1 + 255) / 256), 256, 0, (hipStream_t)stream>>>(dout, w, W, 1, t1, tmp);
  FRTM_LAUNCH_CHECK();
  size_t t2 = (size_t)planes * h * w;                       // rows: (planes, H, w) -> (planes, h, w)
  k_bilinear_bwd_axis<<<(unsigned)((t2 + 255) / 256), 256, 0, (hipStream_t)stream>>>(tmp, h, H, w, t2, din);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_cab_backward_reduce(const float* dout, const float* shallow, int planes, int HW, float* a, float* b, frtm_stream_t stream) {
  FRTM_CHECK_ARG(dout && shallow && a && b && planes > 0 && HW > 0, "frtm_cab_backward_reduce: bad argument");
  k_cab_bwd_reduce<<<planes, 256, 0, (hipStream_t)stream>>>(dout, shallow, HW, a, b);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_cab_gate_backward(const float* sp, const float* dp, const float* gate, const float* a, const float* badd, const float* W1,
                           const float* b1, const float* W2, int n, int oc, float* dW1, float* db1, float* dW2, float* db2, float* dsp,
                           float* ddp, frtm_stream_t stream) {
  FRTM_CHECK_ARG(sp && dp && gate && a && W1 && b1 && W2 && dsp && ddp && n > 0 && oc > 0, "frtm_cab_gate_backward: bad argument");
  const size_t lds = (size_t)5 * n * oc * sizeof(float);
  FRTM_CHECK_ARG(lds <= 65536, "frtm_cab_gate_backward: n * oc = %d too large for one workgroup", n * oc);
  k_cab_gate_bwd<<<1, 256, lds, (hipStream_t)stream>>>(sp, dp, gate, a, badd, W1, b1, W2, n, oc, dW1, db1, dW2, db2, dsp, ddp);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_cab_backward_shallow(const float* dout, const float* gate, const float* dsp, int planes, int HW, float* ds, frtm_stream_t stream) {
  FRTM_CHECK_ARG(dout && gate && dsp && ds && planes > 0 && planes <= 65535 && HW > 0, "frtm_cab_backward_shallow: bad argument");
  k_cab_bwd_shallow<<<dim3(ceil_div(HW, 256), planes), 256, 0, (hipStream_t)stream>>>(dout, gate, dsp, HW, ds);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_add_plane(float* x, const float* v, float scale, int planes, int HW, frtm_stream_t stream) {
  FRTM_CHECK_ARG(x && v && planes > 0 && planes <= 65535 && HW > 0, "frtm_add_plane: bad argument");
  k_add_plane<<<dim3(ceil_div(HW, 256), planes), 256, 0, (hipStream_t)stream>>>(x, v, scale, HW);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_shift9(const float* dl, int n, int H, int W, float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(dl && out && n > 0 && n <= 65535 && H > 0 && W > 0 && (size_t)H * W < 0x7fffffff, "frtm_shift9: bad argument");
  k_shift9<<<dim3(ceil_div(H * W, 256), n), 256, 0, (hipStream_t)stream>>>(dl, H, W, out);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

}  // extern "C"
