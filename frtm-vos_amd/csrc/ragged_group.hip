// The refiner's three per-frame places and the mask merge for frames that carry DIFFERENT numbers of objects (a StreamPool group of
// streams with unequal object counts, model/stream_pool.py).  The refiner is per sample everywhere except
//   * the TSE base map, shared by the objects of a frame          (k_tse_inject of refiner_ops.hip),
//   * the deepest CAB's pooled vector, shared the same way         (k_cab_gate, k_cab_combine),
//   * the merge over a frame's objects                             (k_track_merge of target_model.hip),
// and those four kernels find the frame of sample s as s / group.  Their twins here read it from a device table instead -- the
// frame_of_pair table of frtm_target_apply_grouped, so one table serves the scoring and the refiner -- and the merge reads each frame's
// first sample from the table's prefix sums.  Per sample (per frame, for the merge) the arithmetic is expression for expression that of
// the kernel named: with the table s / group the results are bit-identical, and a sample's result does not depend on what else the
// launch holds.  The table entry is uniform per workgroup (its address depends on blockIdx alone), so it is one scalar load.  A sample
// whose entry names no frame of the batch is skipped and its output left untouched, the rule frtm_target_apply_grouped has for pairs:
// a wrong table reads and writes nothing out of bounds.
#include "frtm_common.h"
#include "resample_taps.h"
#include "../../include/frtm_hip.h"

// k_tse_inject with base[frame_of[n]]: the tile, the channel groups and every expression are that kernel's.
constexpr int RG_INJ_TH = 8, RG_INJ_TW = 32, RG_INJ_CG = 4;
__global__ __launch_bounds__(256) void k_tse_inject_indexed(const float* __restrict__ base, const float* __restrict__ bias,
                                                             const float* __restrict__ ws, const float* __restrict__ scores,
                                                             const int* __restrict__ frame_of, int F, int C, int h, int w, int H, int W,
                                                             float* __restrict__ out) {
  __shared__ float S[RG_INJ_TH + 2][RG_INJ_TW + 2];
  const int n = blockIdx.z / RG_INJ_CG, cg = blockIdx.z % RG_INJ_CG;
  const int frame = frame_of[n];
  if ((unsigned)frame >= (unsigned)F) return;              // (uniform per workgroup, before any barrier)
  base += (size_t)frame * C * H * W;
  const int cper = (C + RG_INJ_CG - 1) / RG_INJ_CG, c_lo = cg * cper, c_hi = min(C, c_lo + cper);
  const int ty0 = blockIdx.y * RG_INJ_TH, tx0 = blockIdx.x * RG_INJ_TW;
  const float* sc = scores + (size_t)n * h * w;
  for (int i = threadIdx.x; i < (RG_INJ_TH + 2) * (RG_INJ_TW + 2); i += 256) {
    const int r = i / (RG_INJ_TW + 2), c = i % (RG_INJ_TW + 2);
    const int y = ty0 - 1 + r, x = tx0 - 1 + c;
    S[r][c] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? bilinear_at(sc, h, w, H, W, y, x) : 0.f;
  }
  __syncthreads();
  const int ly = threadIdx.x / RG_INJ_TW, lx = threadIdx.x % RG_INJ_TW;
  const int y = ty0 + ly, x = tx0 + lx;
  if (y >= H || x >= W) return;
  float s[9];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) s[dy * 3 + dx] = S[ly + dy][lx + dx];
  const size_t HW = (size_t)H * W, pix = (size_t)y * W + x;
  for (int c = c_lo; c < c_hi; ++c) {
    float v = base[c * HW + pix] + bias[c];
#pragma unroll
    for (int k = 0; k < 9; ++k) v += ws[c * 9 + k] * s[k];
    out[((size_t)n * C + c) * HW + pix] = fmaxf(v, 0.f);
  }
}

// k_cab_combine with deeper[entry_of[n]]: one block = RG_CAB_RB rows of one plane.
constexpr int RG_CAB_RB = 16;
__global__ __launch_bounds__(256) void k_cab_combine_indexed(const float* __restrict__ shallow, const float* __restrict__ gate,
                                                              const float* __restrict__ deeper, const int* __restrict__ entry_of, int entries,
                                                              int C, int hd, int wd, int H, int W, float* __restrict__ out) {
  const int pl = blockIdx.y;                                // n * C + c
  const int c = pl % C, n = pl / C;
  const int entry = entry_of[n];
  if ((unsigned)entry >= (unsigned)entries) return;
  const float g = 1.f / (1.f + __expf(-gate[pl]));
  const size_t dn = (size_t)entry;
  const float* __restrict__ dp = deeper + (dn * C + c) * (size_t)hd * wd;
  const float* __restrict__ sp = shallow + (size_t)pl * H * W;
  float* __restrict__ op = out + (size_t)pl * H * W;
  const bool same = (hd == H && wd == W);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int r0 = blockIdx.x * RG_CAB_RB;
  for (int x = tx; x < W; x += 64) {
    int x0, x1; float lx0, lx1;
    bilinear_taps(x, (float)wd / (float)W, wd, x0, x1, lx0, lx1);
    float sv[RG_CAB_RB / 4], dv[RG_CAB_RB / 4];
#pragma unroll
    for (int k = 0; k < RG_CAB_RB / 4; ++k) {
      const int y = min(r0 + ty + 4 * k, H - 1);
      if (same) {
        dv[k] = dp[y * wd + x];
      } else {
        int y0, y1; float ly0, ly1;
        bilinear_taps(y, (float)hd / (float)H, hd, y0, y1, ly0, ly1);
        dv[k] = ly0 * (lx0 * dp[y0 * wd + x0] + lx1 * dp[y0 * wd + x1]) + ly1 * (lx0 * dp[y1 * wd + x0] + lx1 * dp[y1 * wd + x1]);
      }
      sv[k] = sp[y * W + x];
    }
#pragma unroll
    for (int k = 0; k < RG_CAB_RB / 4; ++k) {
      const int y = r0 + ty + 4 * k;
      if (y < H) op[y * W + x] = sv[k] * g + dv[k];
    }
  }
}

// k_cab_gate with dp[row_of[n]]: one block per sample, the same four partial sums per output combined in the same order.
__global__ __launch_bounds__(256) void k_cab_gate_indexed(const float* __restrict__ sp, const float* __restrict__ dp, const int* __restrict__ row_of,
                                                           int rows, const float* __restrict__ W1, const float* __restrict__ b1,
                                                           const float* __restrict__ W2, const float* __restrict__ b2, int oc,
                                                           float* __restrict__ gate) {
  extern __shared__ float sm[];                      // [2oc] input, [oc] hidden, [4][oc] partial sums
  float* v = sm; float* hid = sm + 2 * oc; float* part = sm + 3 * oc;
  const int n = blockIdx.x, tid = threadIdx.x;
  const int row = row_of[n];
  if ((unsigned)row >= (unsigned)rows) return;       // (uniform per workgroup, before any barrier)
  const size_t dn = (size_t)row;
  for (int i = tid; i < 2 * oc; i += 256) v[i] = i < oc ? sp[(size_t)n * oc + i] : dp[dn * oc + i - oc];
  __syncthreads();
  const int q = tid >> 6, lane = tid & 63;
  for (int j0 = 0; j0 < oc; j0 += 64) {
    const int j = j0 + lane;
    const int i0 = q * (2 * oc / 4), i1 = (q + 1) * (2 * oc / 4);
    float a = 0.f;
    if (j < oc) {
#pragma unroll 8
      for (int i = i0; i < i1; ++i) a += v[i] * W1[(size_t)i * oc + j];
      part[q * oc + j] = a;
    }
  }
  __syncthreads();
  for (int j = tid; j < oc; j += 256) hid[j] = fmaxf(b1[j] + ((part[j] + part[oc + j]) + (part[2 * oc + j] + part[3 * oc + j])), 0.f);
  __syncthreads();
  for (int k0 = 0; k0 < oc; k0 += 64) {
    const int k = k0 + lane;
    const int j0 = q * (oc / 4), j1 = (q + 1) * (oc / 4);
    float a = 0.f;
    if (k < oc) {
#pragma unroll 8
      for (int j = j0; j < j1; ++j) a += hid[j] * W2[(size_t)j * oc + k];
      part[q * oc + k] = a;
    }
  }
  __syncthreads();
  for (int k = tid; k < oc; k += 256) gate[(size_t)n * oc + k] = b2[k] + ((part[k] + part[oc + k]) + (part[2 * oc + k] + part[3 * oc + k]));
}

// The ragged merge.  `first` (frames + 1) holds the exclusive prefix sums of the per-frame object counts: frame f reads the logit planes
// first[f] .. first[f+1] - 1 and owns the n_f + 1 mask planes (and counts) from plane first[f] + f on.  A frame is taken only when
// 0 <= first[f], 1 <= n_f <= 15 and first[f+1] <= first[frames]: whatever the table holds, nothing is touched beyond the
// first[frames] logit planes and first[frames] + frames mask planes that the table itself announces.
constexpr int RG_MERGE_MAX = 16;
__device__ __forceinline__ bool ragged_frame(const int* __restrict__ first, int frames, int f, int& a, int& n) {
  a = first[f];
  const int b = first[f + 1];
  n = b - a;
  return a >= 0 && n >= 1 && n < RG_MERGE_MAX && b <= first[frames];
}

// counts of every valid frame to zero (16 threads per frame): the packed size is known on the device only.
__global__ __launch_bounds__(256) void k_ragged_zero_counts(const int* __restrict__ first, int frames, int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int f = i / RG_MERGE_MAX, k = i % RG_MERGE_MAX;
  if (f >= frames) return;
  int a, n;
  if (ragged_frame(first, frames, f, a, n) && k <= n) counts[(size_t)a + f + k] = 0;
}

// k_track_merge without the label decoding, K = n_f + 1 per frame.
__global__ __launch_bounds__(256) void k_track_merge_ragged(const float* __restrict__ logits, const int* __restrict__ first, int frames, int HW,
                                                            float* __restrict__ masks, int* __restrict__ counts, float thr) {
  const int f = blockIdx.y;
  int a, n;
  if (!ragged_frame(first, frames, f, a, n)) return;        // (uniform per workgroup, before any barrier)
  const int K = n + 1;
  logits += (size_t)a * HW;
  masks += ((size_t)a + f) * HW;
  int cnt[RG_MERGE_MAX];
#pragma unroll
  for (int k = 0; k < RG_MERGE_MAX; ++k) cnt[k] = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    float p[RG_MERGE_MAX];
    float bg = INFINITY;
    for (int k = 1; k < K; ++k) {
      const float x = logits[(size_t)(k - 1) * HW + i];
      float v = 1.f / (1.f + expf(-x));                       // torch.sigmoid
      v = fminf(fmaxf(v, 1e-7f), 1.f - 1e-7f);
      p[k] = v;
      bg = fminf(bg, 1.f - v);
    }
    p[0] = bg;
    float mx = -INFINITY; int arg = 0;
    for (int k = 0; k < K; ++k) { p[k] = p[k] / (1.f - p[k]); if (p[k] > mx) { mx = p[k]; arg = k; } }
    float den = 0.f;
    for (int k = 0; k < K; ++k) { p[k] = expf(p[k] - mx); den += p[k]; }
    const float win = p[arg] / den;
    for (int k = 0; k < K; ++k) masks[(size_t)k * HW + i] = (k == arg) ? win : 0.f;
    if (win > thr) {
#pragma unroll
      for (int k = 0; k < RG_MERGE_MAX; ++k) cnt[k] += (k == arg) ? 1 : 0;
    }
  }
  if (counts) {
    __shared__ int wsum[4][RG_MERGE_MAX];
    for (int k = 0; k < K; ++k) {
      int c = cnt[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
      if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][k] = c;
    }
    __syncthreads();
    if (threadIdx.x < K) {
      const int tot = (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
      if (tot) atomicAdd(&counts[(size_t)a + f + threadIdx.x], tot);       // integer atomics: order independent
    }
  }
}

extern "C" {

int frtm_tse_inject_indexed(const float* base, const float* bias, const float* ws, const float* scores, int n, const int* frame_of, int F,
                            int C, int h, int w, int H, int W, float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(base && bias && ws && scores && frame_of && out && n > 0 && C > 0 && F > 0, "frtm_tse_inject_indexed: bad argument");
  FRTM_CHECK_ARG(h > 0 && w > 0 && H > 0 && W > 0, "frtm_tse_inject_indexed: map sizes must be positive (scores %d x %d, maps %d x %d)", h, w, H, W);
  FRTM_CHECK_ARG((size_t)H * W < 0x7fffffff && (size_t)h * w < 0x7fffffff, "frtm_tse_inject_indexed: map too large");
  FRTM_CHECK_ARG((size_t)n * RG_INJ_CG <= 65535, "frtm_tse_inject_indexed: at most %d samples per call (got %d)", 65535 / RG_INJ_CG, n);
  FRTM_CHECK_ARG(ceil_div(H, RG_INJ_TH) <= 65535, "frtm_tse_inject_indexed: at most %d rows per map (got %d)", 65535 * RG_INJ_TH, H);
  dim3 g(ceil_div(W, RG_INJ_TW), ceil_div(H, RG_INJ_TH), n * RG_INJ_CG);
  k_tse_inject_indexed<<<g, 256, 0, (hipStream_t)stream>>>(base, bias, ws, scores, frame_of, F, C, h, w, H, W, out);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_cab_gate_indexed(const float* sp, const float* dp, const int* row_of, int rows, const float* W1, const float* b1, const float* W2,
                          const float* b2, int n, int oc, float* gate, frtm_stream_t stream) {
  FRTM_CHECK_ARG(sp && dp && row_of && W1 && b1 && W2 && b2 && gate && n > 0 && oc > 0 && rows > 0, "frtm_cab_gate_indexed: bad argument");
  // 7 oc floats of dynamic LDS; 64 KB is what a launch gets without raising the kernel's limit
  FRTM_CHECK_ARG((size_t)7 * oc * sizeof(float) <= 65536, "frtm_cab_gate_indexed: oc = %d needs %zu bytes of LDS, more than the 65536 of a default launch",
                 oc, (size_t)7 * oc * sizeof(float));
  FRTM_CHECK_ARG(oc % 4 == 0, "frtm_cab_gate_indexed: oc must be a multiple of 4 (got %d)", oc);
  k_cab_gate_indexed<<<n, 256, 7 * oc * sizeof(float), (hipStream_t)stream>>>(sp, dp, row_of, rows, W1, b1, W2, b2, oc, gate);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_cab_combine_indexed(const float* shallow, const float* gate, const float* deeper, const int* entry_of, int entries, int n, int C,
                             int hd, int wd, int H, int W, float* out, frtm_stream_t stream) {
  FRTM_CHECK_ARG(shallow && gate && deeper && entry_of && out && n > 0 && C > 0 && entries > 0, "frtm_cab_combine_indexed: bad argument");
  FRTM_CHECK_ARG(hd > 0 && wd > 0 && H > 0 && W > 0, "frtm_cab_combine_indexed: map sizes must be positive (deeper %d x %d, maps %d x %d)", hd, wd, H, W);
  FRTM_CHECK_ARG((size_t)n * C <= 65535 && (size_t)H * W < 0x7fffffff && (size_t)hd * wd < 0x7fffffff,
                 "frtm_cab_combine_indexed: at most 65535 planes per call");
  dim3 g(ceil_div(H, RG_CAB_RB), n * C);
  k_cab_combine_indexed<<<g, 256, 0, (hipStream_t)stream>>>(shallow, gate, deeper, entry_of, entries, C, hd, wd, H, W, out);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_track_merge_ragged(const float* logits, int frames, const int* first, int HW, float* masks, int* counts, float thr,
                            frtm_stream_t stream) {
  FRTM_CHECK_ARG(logits && first && masks && HW > 0, "frtm_track_merge_ragged: bad argument");
  FRTM_CHECK_ARG(frames > 0 && frames <= 65535, "frtm_track_merge_ragged: needs 1 <= frames <= 65535 (got %d)", frames);
  hipStream_t st = (hipStream_t)stream;
  if (counts) {
    k_ragged_zero_counts<<<ceil_div(frames * RG_MERGE_MAX, 256), 256, 0, st>>>(first, frames, counts);
    FRTM_LAUNCH_CHECK();
  }
  dim3 g(min(ceil_div(HW, 256 * 4), 256), frames);
  k_track_merge_ragged<<<g, 256, 0, st>>>(logits, first, frames, HW, masks, counts, thr);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

}  // extern "C"
