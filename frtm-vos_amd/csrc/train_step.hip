// The two ends of a refiner training step that sit between the HIP backward and the next HIP forward (model/train_loss.py,
// lib/fused_adam.py): the loss tail on the logits and the optimiser update.  Both are bandwidth-bound streaming kernels: 16-byte
// accesses on the aligned body, scalar head / tail, wave sums before LDS, no atomics of any kind.
//
//   k_bce_logits   one pass over the logits z and targets t of N samples: per pixel, in fp32,
//                    term = t * min(softplus(-z), 100) + (1 - t) * min(softplus(z), 100),   softplus(x) = max(x, 0) + log1p(exp(-|x|))
//                    dz   = (sigmoid(z) - t) / (N * HW)     (the part of a term whose clamp binds contributes no gradient)
//                  and the two integer counts of mask_iou, (z > 0) & (t > 0.5) and (z > 0) | (t > 0.5).  grid = (P, N): workgroup
//                  (j, n) strides over sample n and leaves one fp64 partial of the loss and two int32 partials in the workspace.
//   k_bce_final    one workgroup: a wave per sample adds its P partials (lane l takes l, l + 64, ... in index order, then the xor tree),
//                  wave 0 then adds the N sample sums the same way.  The order is a function of (N, HW) alone, so two calls agree
//                  bit for bit.
//   k_scale_by     dz *= the loss's incoming gradient, a device scalar (autograd's chain rule without a read-back).
//   k_adam         torch.optim.Adam's update (weight_decay folded into the gradient, optional AMSGrad) over a device table of
//                  tensors; a workgroup takes chunks of ADAM_CHUNK elements of one tensor, so one launch covers a parameter group.
#include "frtm_common.h"
#include "../../include/frtm_hip.h"
#include <cstdint>

#define BCE_THREADS 256
#define BCE_MAX_BLOCKS 2048        // grid cap of a memory-bound launch (256 CUs x 8 workgroups); the rest is strided
#define BCE_CLAMP 100.f            // -log clamp of torch's BCELoss
#define ADAM_CHUNK 2048            // elements per table chunk: 256 threads x two 16-byte accesses per array

static int bce_parts(int N, long long HW) {
  long long want = (HW + 4LL * BCE_THREADS - 1) / (4LL * BCE_THREADS);
  long long cap = BCE_MAX_BLOCKS / N;
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  return (int)(want < 1 ? 1 : want);
}

struct BceAcc {
  double loss;
  int inter, uni;
};

// one pixel: accumulates, returns dz (already divided by the pixel count).  The kernel has to stay under ~50 VALU instructions per
// pixel to run at the HBM rate, so exp, log and the reciprocal are the hardware's (1 ulp each) instead of the library's; log1p(e) keeps
// its accuracy for small e through the rounding error of u = 1 + e, which is known exactly: log1p(e) = log(u) + (e - (u - 1)) / u.
__device__ __forceinline__ float bce_pixel(float z, float t, float inv_total, BceAcc& a) {
  const float az = fabsf(z);
  const float e = __expf(-az);                     // in [0, 1]
  const float u = 1.f + e;
  const float r = __builtin_amdgcn_rcpf(u);
  const float l = __logf(u) + (e - (u - 1.f)) * r; // log1p(e)
  const float sp_pos = fmaxf(z, 0.f) + l;          // softplus(z)  = -log(1 - sigmoid(z))
  const float sp_neg = fmaxf(-z, 0.f) + l;         // softplus(-z) = -log(sigmoid(z))
  const bool c_pos = sp_pos > BCE_CLAMP, c_neg = sp_neg > BCE_CLAMP;
  const float term = t * (c_neg ? BCE_CLAMP : sp_neg) + (1.f - t) * (c_pos ? BCE_CLAMP : sp_pos);
  a.loss += (double)term;
  const bool p = z > 0.f, g = t > 0.5f;
  a.inter += (p && g) ? 1 : 0;
  a.uni += (p || g) ? 1 : 0;
  const float big = r, small = e * r;              // sigmoid(|z|), sigmoid(-|z|)
  const float sig = z >= 0.f ? big : small, one_m_sig = z >= 0.f ? small : big;
  float d = sig - t;
  if (c_pos || c_neg) d = (c_pos ? 0.f : (1.f - t) * sig) - (c_neg ? 0.f : t * one_m_sig);
  return d * inv_total;
}

__device__ __forceinline__ float bce_target(const float* t, size_t i) { return t[i]; }
__device__ __forceinline__ float bce_target(const unsigned char* t, size_t i) { return (float)t[i]; }
__device__ __forceinline__ float4 bce_target4(const float* t, size_t i) { return *reinterpret_cast<const float4*>(t + i); }
__device__ __forceinline__ float4 bce_target4(const unsigned char* t, size_t i) {
  const unsigned w = *reinterpret_cast<const unsigned*>(t + i);
  return make_float4((float)(w & 255u), (float)((w >> 8) & 255u), (float)((w >> 16) & 255u), (float)(w >> 24));
}

// z, dz and (fp32) t are 16-byte aligned at element 0, uint8 t 4-byte aligned: element index % 4 == 0 is the aligned body of all of them.
template <typename TT>
__global__ __launch_bounds__(BCE_THREADS) void k_bce_logits(const float* __restrict__ z, const TT* __restrict__ t, int HW, float inv_total,
                                                            float* __restrict__ dz, double* __restrict__ part_loss, int* __restrict__ part_cnt) {
  const int n = blockIdx.y, j = blockIdx.x, P = gridDim.x;
  const size_t base = (size_t)n * HW;
  const int head = min((int)((4 - (base & 3)) & 3), HW);            // scalar pixels before the first aligned one
  const int nvec = (HW - head) >> 2;
  const int tail0 = head + 4 * nvec;
  BceAcc a = {0.0, 0, 0};
  for (int q = j * BCE_THREADS + threadIdx.x; q < nvec; q += P * BCE_THREADS) {
    const size_t i = base + head + 4 * (size_t)q;
    const float4 zv = *reinterpret_cast<const float4*>(z + i);
    const float4 tv = bce_target4(t, i);
    float4 d;
    d.x = bce_pixel(zv.x, tv.x, inv_total, a);
    d.y = bce_pixel(zv.y, tv.y, inv_total, a);
    d.z = bce_pixel(zv.z, tv.z, inv_total, a);
    d.w = bce_pixel(zv.w, tv.w, inv_total, a);
    if (dz) *reinterpret_cast<float4*>(dz + i) = d;
  }
  if (j == 0) {                                                      // at most 3 + 3 pixels per sample
    const int k = threadIdx.x;
    const int rest = head + (HW - tail0);
    if (k < rest) {
      const size_t i = base + (k < head ? k : tail0 + (k - head));
      const float d = bce_pixel(z[i], bce_target(t, i), inv_total, a);
      if (dz) dz[i] = d;
    }
  }
  __shared__ double red_l[BCE_THREADS / 64];
  __shared__ int red_c[2][BCE_THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a.loss += __shfl_xor(a.loss, off, 64);
    a.inter += __shfl_xor(a.inter, off, 64);
    a.uni += __shfl_xor(a.uni, off, 64);
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { red_l[wv] = a.loss; red_c[0][wv] = a.inter; red_c[1][wv] = a.uni; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const size_t o = (size_t)n * P + j;
    part_loss[o] = (red_l[0] + red_l[1]) + (red_l[2] + red_l[3]);
    part_cnt[2 * o] = (red_c[0][0] + red_c[0][1]) + (red_c[0][2] + red_c[0][3]);
    part_cnt[2 * o + 1] = (red_c[1][0] + red_c[1][1]) + (red_c[1][2] + red_c[1][3]);
  }
}

// lanes of a wave take a list's entries l, l + 64, ... in order, then the xor tree: a fixed order for a given length
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(256) void k_bce_final(const double* __restrict__ part_loss, const int* __restrict__ part_cnt, int N, int P,
                                                   double inv_total, double* sample_loss, float* __restrict__ loss,
                                                   int* __restrict__ inter, int* __restrict__ uni) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int n = wv; n < N; n += 4) {                                   // one wave per sample
    double s = 0.0;
    int ci = 0, cu = 0;
    for (int j = lane; j < P; j += 64) {
      const size_t o = (size_t)n * P + j;
      s += part_loss[o];
      ci += part_cnt[2 * o];
      cu += part_cnt[2 * o + 1];
    }
    s = wave_sum_f64(s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      ci += __shfl_xor(ci, off, 64);
      cu += __shfl_xor(cu, off, 64);
    }
    if (lane == 0) {
      sample_loss[n] = s;
      inter[n] = ci;
      uni[n] = cu;
    }
  }
  __syncthreads();                                                   // (one workgroup: its own global writes are visible after the barrier)
  if (wv == 0) {
    double s = 0.0;
    for (int n = lane; n < N; n += 64) s += sample_loss[n];
    s = wave_sum_f64(s);
    if (lane == 0) loss[0] = (float)(s * inv_total);
  }
}

// x *= s[0], s on the device: the chain rule through the scalar loss without reading the incoming gradient back to the host
__global__ __launch_bounds__(256) void k_scale_by(float* __restrict__ x, size_t n, const float* __restrict__ s) {
  const float a = s[0];
  const size_t nvec = n >> 2, stride = (size_t)gridDim.x * 256;
  for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < nvec; q += stride) {
    float4 v = reinterpret_cast<float4*>(x)[q];
    v.x *= a; v.y *= a; v.z *= a; v.w *= a;
    reinterpret_cast<float4*>(x)[q] = v;
  }
  const size_t i = 4 * nvec + threadIdx.x;
  if (blockIdx.x == 0 && i < n) x[i] *= a;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Adam / AMSGrad
// ---------------------------------------------------------------------------------------------------------------------------------
// (pointers read from a table are generic to the compiler: naming the global address space keeps the accesses global_load / global_store)
typedef __attribute__((address_space(1))) float gfloat;
typedef float vfloat4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) vfloat4 gfloat4;

struct AdamTensor {            // eight 64-bit words per tensor (lib/fused_adam.py builds the table)
  gfloat* p;
  const gfloat* g;
  gfloat* m;
  gfloat* v;
  gfloat* vmax;                // unused without AMSGrad
  long long n;
  long long vec;               // 1: the five pointers are 16-byte aligned
  long long pad;
};

struct AdamArgs {
  float step, bc2_sqrt, b1, b2, one_m_b1, one_m_b2, eps, wd;      // 1 - beta rounded once from double, as torch passes them
};

template <bool AMS>
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float& vmax, const AdamArgs& c) {
  g = g + c.wd * p;
  m = c.b1 * m + c.one_m_b1 * g;
  v = c.b2 * v + c.one_m_b2 * g * g;
  float s = v;
  if (AMS) { vmax = fmaxf(vmax, v); s = vmax; }
  p = p - c.step * (m / (sqrtf(s) / c.bc2_sqrt + c.eps));
}

template <bool AMS>
__global__ __launch_bounds__(256) void k_adam(const AdamTensor* __restrict__ tens, int ntens, const int2* __restrict__ chunks, int nchunks,
                                              AdamArgs c) {
  for (int ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int2 cd = chunks[ch];                                       // (tensor, chunk index within it)
    if (cd.x < 0 || cd.x >= ntens || cd.y < 0) continue;
    const AdamTensor T = tens[cd.x];
    const long long off = (long long)cd.y * ADAM_CHUNK;
    if (off >= T.n) continue;
    const int len = (int)min((long long)ADAM_CHUNK, T.n - off);
    gfloat* p = T.p + off;
    const gfloat* g = T.g + off;
    gfloat* m = T.m + off;
    gfloat* v = T.v + off;
    gfloat* vm = AMS ? T.vmax + off : nullptr;
    const int nvec = T.vec ? len >> 2 : 0;                            // (off is a multiple of 4: the chunk keeps the tensor's alignment)
    for (int q = threadIdx.x; q < nvec; q += 256) {
      vfloat4 pv = ((gfloat4*)p)[q];
      const vfloat4 gv = ((const gfloat4*)g)[q];
      vfloat4 mv = ((gfloat4*)m)[q];
      vfloat4 vv = ((gfloat4*)v)[q];
      vfloat4 xv = {0.f, 0.f, 0.f, 0.f};
      if (AMS) xv = ((gfloat4*)vm)[q];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float pe = pv[k], me = mv[k], ve = vv[k], xe = xv[k];
        adam_elem<AMS>(pe, gv[k], me, ve, xe, c);
        pv[k] = pe; mv[k] = me; vv[k] = ve; xv[k] = xe;
      }
      ((gfloat4*)p)[q] = pv;
      ((gfloat4*)m)[q] = mv;
      ((gfloat4*)v)[q] = vv;
      if (AMS) ((gfloat4*)vm)[q] = xv;
    }
    for (int i = 4 * nvec + threadIdx.x; i < len; i += 256) {
      float pe = p[i], me = m[i], ve = v[i], xe = AMS ? vm[i] : 0.f;
      adam_elem<AMS>(pe, g[i], me, ve, xe, c);
      p[i] = pe;
      m[i] = me;
      v[i] = ve;
      if (AMS) vm[i] = xe;
    }
  }
}

extern "C" {

size_t frtm_bce_logits_workspace_bytes(int N, int H, int W) {
  if (N < 1 || H < 1 || W < 1) return 0;
  const size_t P = (size_t)bce_parts(N, (long long)H * W);
  return (size_t)N * P * (sizeof(double) + 2 * sizeof(int)) + (size_t)N * sizeof(double);
}

int frtm_bce_logits(const float* logits, const void* target, int target_bytes, int N, int H, int W, float* dlogits, float* loss, int* inter,
                    int* uni, void* ws, size_t ws_bytes, frtm_stream_t stream) {
  FRTM_CHECK_ARG(logits && target && loss && inter && uni && ws, "frtm_bce_logits: null argument");
  FRTM_CHECK_ARG(target_bytes == 1 || target_bytes == 4, "frtm_bce_logits: target_bytes must be 1 (uint8) or 4 (float), got %d", target_bytes);
  FRTM_CHECK_ARG(N >= 1 && H >= 1 && W >= 1, "frtm_bce_logits: N, H, W must be >= 1 (got %d, %d, %d)", N, H, W);
  FRTM_CHECK_ARG(N <= 65535 && (long long)H * W < (1LL << 31) - (1LL << 23),
                 "frtm_bce_logits: N = %d above 65535 or H * W = %d * %d too large", N, H, W);
  FRTM_CHECK_ARG(((uintptr_t)logits & 15) == 0 && ((uintptr_t)dlogits & 15) == 0 && ((uintptr_t)target & (target_bytes == 4 ? 15 : 3)) == 0 &&
                     ((uintptr_t)ws & 7) == 0,
                 "frtm_bce_logits: logits, dlogits and float targets must be 16-byte aligned (uint8 targets 4-byte, workspace 8-byte)");
  FRTM_CHECK_ARG(ws_bytes >= frtm_bce_logits_workspace_bytes(N, H, W), "frtm_bce_logits: workspace of %zu bytes, need %zu", ws_bytes,
                 frtm_bce_logits_workspace_bytes(N, H, W));
  hipStream_t st = (hipStream_t)stream;
  const int HW = H * W, P = bce_parts(N, HW);
  const double total = (double)N * (double)HW;
  double* part_loss = (double*)ws;
  double* sample_loss = part_loss + (size_t)N * P;
  int* part_cnt = (int*)(sample_loss + N);
  dim3 grid(P, N);
  if (target_bytes == 1)
    k_bce_logits<unsigned char><<<grid, BCE_THREADS, 0, st>>>(logits, (const unsigned char*)target, HW, (float)(1.0 / total), dlogits, part_loss, part_cnt);
  else
    k_bce_logits<float><<<grid, BCE_THREADS, 0, st>>>(logits, (const float*)target, HW, (float)(1.0 / total), dlogits, part_loss, part_cnt);
  FRTM_LAUNCH_CHECK();
  k_bce_final<<<1, 256, 0, st>>>(part_loss, part_cnt, N, P, 1.0 / total, sample_loss, loss, inter, uni);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_scale_by(float* x, size_t n, const float* scale, frtm_stream_t stream) {
  FRTM_CHECK_ARG(x && scale, "frtm_scale_by: null argument");
  FRTM_CHECK_ARG(((uintptr_t)x & 15) == 0, "frtm_scale_by: x must be 16-byte aligned");
  if (n == 0) return FRTM_OK;
  const size_t want = (n / 4 + 255) / 256;
  const int grid = (int)(want < 1 ? 1 : want > BCE_MAX_BLOCKS ? BCE_MAX_BLOCKS : want);
  k_scale_by<<<grid, 256, 0, (hipStream_t)stream>>>(x, n, scale);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_adam_chunk_elems(void) { return ADAM_CHUNK; }

int frtm_adam_amsgrad(const void* tensors, int ntensors, const void* chunks, int nchunks, double lr, double bias_correction1,
                      double bias_correction2, double beta1, double beta2, double eps, double weight_decay, int amsgrad, frtm_stream_t stream) {
  FRTM_CHECK_ARG(tensors && chunks, "frtm_adam_amsgrad: null table");
  FRTM_CHECK_ARG(ntensors >= 1 && nchunks >= ntensors, "frtm_adam_amsgrad: %d tensors in %d chunks", ntensors, nchunks);
  FRTM_CHECK_ARG(((uintptr_t)tensors & 7) == 0 && ((uintptr_t)chunks & 7) == 0, "frtm_adam_amsgrad: tables must be 8-byte aligned");
  FRTM_CHECK_ARG(bias_correction1 > 0.0 && bias_correction2 > 0.0, "frtm_adam_amsgrad: bias corrections must be positive (got %g, %g)",
                 bias_correction1, bias_correction2);
  AdamArgs c;
  c.step = (float)(lr / bias_correction1);
  c.bc2_sqrt = (float)sqrt(bias_correction2);
  c.b1 = (float)beta1;
  c.b2 = (float)beta2;
  c.one_m_b1 = (float)(1.0 - beta1);
  c.one_m_b2 = (float)(1.0 - beta2);
  c.eps = (float)eps;
  c.wd = (float)weight_decay;
  hipStream_t st = (hipStream_t)stream;
  const int grid = min(nchunks, BCE_MAX_BLOCKS);
  if (amsgrad)
    k_adam<true><<<grid, 256, 0, st>>>((const AdamTensor*)tensors, ntensors, (const int2*)chunks, nchunks, c);
  else
    k_adam<false><<<grid, 256, 0, st>>>((const AdamTensor*)tensors, ntensors, (const int2*)chunks, nchunks, c);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

}  // extern "C"
