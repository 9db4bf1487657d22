// The four places where the refiner and the tracker's tail are per FRAME rather than per sample, each defined once:
//   * the TSE base map, shared by the objects of a frame           (tse_inject_body),
//   * the deepest CAB's pooled vector in its gate and its combine  (cab_gate_body, cab_combine_body),
//   * the merge over a frame's objects                             (track_merge_body).
// A body is a template over how a frame is found: from `s / group` (refiner_ops.hip, target_model.hip: every frame has the same
// number of objects) or from a device table (ragged_group.hip: any mix of counts).  Both instances run the same expressions per sample,
// so a stream's bits do not depend on which one served it.  The __global__ kernels are wrappers in those files.
#pragma once
#include "frtm_common.h"
#include "resample_taps.h"

constexpr int INJ_TH = 8;      // tile = 8 rows x 32 columns: every half wave writes a 128-byte row segment (16 x 16 tiles: 64-byte segments,
constexpr int INJ_TW = 32;     // 46 us for the 120 x 214 level of 10 samples)
constexpr int INJ_CG = 4;      // channel groups per object (more workgroups on the small maps)
constexpr int CAB_RB = 16;     // rows of one plane per block: 64 x 4 threads, every thread 4 rows of its columns
constexpr int MERGE_MAX = 16;  // planes of one frame (background + 15 objects) that the merge and the way back to the native size hold per thread

// ---- the label of one pixel of a MERGED mask stack (every plane but the winner is 0), defined once for the way back to the native size
// (native_size.hip) and the renderer (frame_render.hip):
//   arg = the first k with the largest m_k (planes offered in order 0, 1, ...; a NaN never wins), plane = arg if arg >= 1 and m_arg > 0.5f, else 0
__device__ __forceinline__ void merged_offer(float m, int k, float& best, int& arg) {
  if (m > best) { best = m; arg = k; }
}
__device__ __forceinline__ int merged_plane(int arg, float best) { return (arg >= 1 && best > 0.5f) ? arg : 0; }

// ---- which frame does sample n belong to?  (passed by value; false: the sample is skipped, before any barrier) ----
struct FrameByGroup {          // `group` consecutive samples (the objects of one frame) share a frame
  int group;
  __device__ __forceinline__ bool operator()(int n, int& f) const { f = n / group; return true; }
};
struct FrameByGroupOrOwn {     // group = 0: one entry per sample
  int group;
  __device__ __forceinline__ bool operator()(int n, int& f) const { f = group > 0 ? n / group : n; return true; }
};
// The entry's address depends on blockIdx alone, so it is one scalar load per workgroup.  An entry that names no frame of the batch
// skips the sample and leaves its output untouched, the rule frtm_target_apply_grouped has for pairs: a wrong table reads and writes
// nothing out of bounds.
struct FrameByTable {
  const int* __restrict__ table;
  int F;
  __device__ __forceinline__ bool operator()(int n, int& f) const { f = table[n]; return (unsigned)f < (unsigned)F; }
};

// TSE score injection (seg_network.py:16-21: h = cat(reduce(ft), interpolate(score)); transform[0]; relu).  The 3x3 conv over
// the 64 feature channels does not depend on the object and arrives pre-computed in `base` (frames,C,H,W); this adds the
// contribution of the one score channel, the bias and the ReLU:
//   out[n,c,y,x] = relu(base[frame(n),c,y,x] + bias[c] + sum_{dy,dx} ws[c,dy,dx] * S_n(y+dy-1, x+dx-1)),  S_n = bilinear(scores[n]) (0 outside)
template <class FrameOf>
__device__ __forceinline__ void tse_inject_body(const float* __restrict__ base, const float* __restrict__ bias, const float* __restrict__ ws,
                                                const float* __restrict__ scores, FrameOf frame_of, int C, int h, int w, int H, int W,
                                                float* __restrict__ out) {
  __shared__ float S[INJ_TH + 2][INJ_TW + 2];
  const int n = blockIdx.z / INJ_CG, cg = blockIdx.z % INJ_CG;
  int frame;
  if (!frame_of(n, frame)) return;
  base += (size_t)frame * C * H * W;
  const int cper = (C + INJ_CG - 1) / INJ_CG, c_lo = cg * cper, c_hi = min(C, c_lo + cper);
  const int ty0 = blockIdx.y * INJ_TH, tx0 = blockIdx.x * INJ_TW;
  const float* sc = scores + (size_t)n * h * w;
  for (int i = threadIdx.x; i < (INJ_TH + 2) * (INJ_TW + 2); i += 256) {
    const int r = i / (INJ_TW + 2), c = i % (INJ_TW + 2);
    const int y = ty0 - 1 + r, x = tx0 - 1 + c;
    S[r][c] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? bilinear_at(sc, h, w, H, W, y, x) : 0.f;
  }
  __syncthreads();
  const int ly = threadIdx.x / INJ_TW, lx = threadIdx.x % INJ_TW;
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

// CAB combine (seg_network.py:38-41): out = shallower * sigmoid(gate[n,c]) + bilinear(deeper[frame(n),c], (hd,wd) -> (H,W)).
// One block = CAB_RB rows of ONE plane: the sigmoid of the gate once per thread, the column taps once per column, the row taps once per
// row -- the element-wise form (64-bit index arithmetic, an exponential and both tap sets per element) ran at 2.1 TB/s on the
// 120 x 214 level.  Same expressions as bilinear_at, so the results are unchanged.
template <class FrameOf>
__device__ __forceinline__ void cab_combine_body(const float* __restrict__ shallow, const float* __restrict__ gate, const float* __restrict__ deeper,
                                                 FrameOf frame_of, int C, int hd, int wd, int H, int W, float* __restrict__ out) {
  const int pl = blockIdx.y;                                // n * C + c
  const int c = pl % C, n = pl / C;
  int frame;
  if (!frame_of(n, frame)) return;
  const float g = 1.f / (1.f + __expf(-gate[pl]));
  const size_t dn = (size_t)frame;
  const float* __restrict__ dp = deeper + (dn * C + c) * (size_t)hd * wd;
  const float* __restrict__ sp = shallow + (size_t)pl * H * W;
  float* __restrict__ op = out + (size_t)pl * H * W;
  const bool same = (hd == H && wd == W);
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int r0 = blockIdx.x * CAB_RB;
  for (int x = tx; x < W; x += 64) {
    int x0, x1; float lx0, lx1;
    bilinear_taps(x, (float)wd / (float)W, wd, x0, x1, lx0, lx1);
    float sv[CAB_RB / 4], dv[CAB_RB / 4];
#pragma unroll
    for (int k = 0; k < CAB_RB / 4; ++k) {                  // all loads of the thread's four rows first (independent), then the stores
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
    for (int k = 0; k < CAB_RB / 4; ++k) {
      const int y = r0 + ty + 4 * k;
      if (y < H) op[y * W + x] = sv[k] * g + dv[k];
    }
  }
}

// Channel-attention gate (seg_network.py:34-37): gate[n,:] = W2^T relu(W1^T [sp[n]; dp[frame(n)]] + b1) + b2 (the sigmoid is applied by
// the combine).  sp / dp: pooled shallower / deeper features (n,oc) / (frames,oc).  W1 (2oc,oc), W2 (oc,oc) are the 1x1 conv weights
// transposed to [in][out].  One block per object: four framework launches (cat, addmm, relu, addmm) become one.  7 oc floats of dynamic LDS.
template <class FrameOf>
__device__ __forceinline__ void cab_gate_body(const float* __restrict__ sp, const float* __restrict__ dp, FrameOf frame_of,
                                              const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
                                              const float* __restrict__ b2, int oc, float* __restrict__ gate) {
  extern __shared__ float sm[];                      // [2oc] input, [oc] hidden, [4][oc] partial sums
  float* v = sm; float* hid = sm + 2 * oc; float* part = sm + 3 * oc;
  const int n = blockIdx.x, tid = threadIdx.x;
  int frame;
  if (!frame_of(n, frame)) return;
  const size_t dn = frame;
  for (int i = tid; i < 2 * oc; i += 256) v[i] = i < oc ? sp[(size_t)n * oc + i] : dp[dn * oc + i - oc];
  __syncthreads();
  // each output is summed by 4 threads over a quarter of the inputs (independent loads in flight), then combined in fixed order
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

// ---- where are frame f's planes?  logit0: its first logit plane; plane0: its first mask plane and count; n: its objects ----
struct UniformFrames {         // n objects in every frame
  int n;
  __device__ __forceinline__ bool operator()(int f, size_t& logit0, size_t& plane0, int& n_f) const {
    n_f = n;
    logit0 = (size_t)f * n;
    plane0 = (size_t)f * (n + 1);
    return true;
  }
};
// `first` (frames + 1) holds the exclusive prefix sums of the per-frame object counts: frame f reads the logit planes
// first[f] .. first[f+1] - 1 and owns the n_f + 1 mask planes (and counts) from plane first[f] + f on.  A frame is taken only when
// 0 <= first[f], 1 <= n_f <= 15 and first[f+1] <= first[frames]: whatever the table holds, nothing is touched beyond the
// first[frames] logit planes and first[frames] + frames mask planes that the table itself announces.
struct RaggedFrames {
  const int* __restrict__ first;
  int frames;
  __device__ __forceinline__ bool operator()(int f, size_t& logit0, size_t& plane0, int& n_f) const {
    const int a = first[f], b = first[f + 1];
    n_f = b - a;
    logit0 = (size_t)a;
    plane0 = (size_t)a + f;
    return a >= 0 && n_f >= 1 && n_f < MERGE_MAX && b <= first[frames];
  }
};

// The tail of Tracker.track for a whole window of frames in ONE pass (reference model/tracker.py:200-221 + the label decoding of
// run_sequence, :143-150 + the pixel counts Discriminator.update's early-out needs, discriminator.py:214):
//   logits (n_f, HW) of the refiner  ->  sigmoid  ->  merge (clamp, background = min(1 - p), soft-max of p / (1 - p), arg-max keeps one
//   plane)  ->  masks (n_f+1, HW)  +  counts[k] = #{masks > thr}  +  labels (frames, HW) uint8 = lut[decode(masks)], when labels != null
// where decode is the reference's: one object: masks[1] > 0.5; several: the same merge applied to the MERGED masks, arg-max.
// Replaces sigmoid + repeat + n plane copies + merge + count + clone + merge + argmax + index (ATen launches) of the window.
// blockIdx.y = frame; a frame that the layout refuses is left untouched.
template <class Frames>
__device__ __forceinline__ void track_merge_body(const float* __restrict__ logits, Frames frames, int HW, float* __restrict__ masks,
                                                 unsigned char* __restrict__ labels, const unsigned char* __restrict__ lut, int single,
                                                 int* __restrict__ counts, float thr) {
  const int f = blockIdx.y;
  size_t logit0, plane0;
  int n;
  if (!frames(f, logit0, plane0, n)) return;                // (uniform per workgroup, before any barrier)
  const int K = n + 1;
  logits += logit0 * HW;
  masks += plane0 * HW;
  int cnt[MERGE_MAX];
#pragma unroll
  for (int k = 0; k < MERGE_MAX; ++k) cnt[k] = 0;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
    float p[MERGE_MAX];
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
      for (int k = 0; k < MERGE_MAX; ++k) cnt[k] += (k == arg) ? 1 : 0;
    }
    if (labels) {
      int lab;
      if (single) lab = (arg == 1 && win > 0.5f) ? 1 : 0;     // :145  object_ids[(masks[1:2] > 0.5)]
      else {
        // :147-150 on the merged masks: every plane but `arg` is 0 -> 1e-7 after the clamp
        const float v = fminf(fmaxf(win, 1e-7f), 1.f - 1e-7f), z = 1e-7f;
        float b2 = INFINITY;
        for (int k = 1; k < K; ++k) b2 = fminf(b2, 1.f - ((k == arg) ? v : z));
        float m2 = -INFINITY; lab = 0;
        for (int k = 0; k < K; ++k) {
          const float q = (k == 0) ? b2 : ((k == arg) ? v : z);
          const float o = q / (1.f - q);
          if (o > m2) { m2 = o; lab = k; }
        }
      }
      labels[(size_t)f * HW + i] = lut[lab];
    }
  }
  if (counts) {
    __shared__ int wsum[4][MERGE_MAX];
    for (int k = 0; k < K; ++k) {
      int c = cnt[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
      if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6][k] = c;
    }
    __syncthreads();
    if (threadIdx.x < K) {
      const int tot = (wsum[0][threadIdx.x] + wsum[1][threadIdx.x]) + (wsum[2][threadIdx.x] + wsum[3][threadIdx.x]);
      if (tot) atomicAdd(&counts[plane0 + threadIdx.x], tot);       // integer atomics: order independent
    }
  }
}
