// DAVIS region (J) and boundary (F) measures as exact integer counts on the device (lib/davis.py: db_eval_iou, seg2bmap,
// db_eval_boundary).  Per (frame, object) six integers: inter, union, n_fg, n_gt, fg_match, gt_match; the host turns them into
// J and F with the same float64 expressions as the numpy path, so both paths agree bit for bit.
//
//   pass 1  k_jf_planes   one read of both label maps for up to JF_IDS ids: per 64 pixels of a row the wave's ballot IS the row
//                         segment of the boundary map (one 64-bit word); the four popcount sums ride in lanes (lane 4 * k + c).
//   pass 2  k_jf_match    one thread per word of a boundary plane; words without a boundary pixel (most) leave at once.  The disk
//                         {dy^2 + dx^2 <= r^2} is the union over dy of row y + dy dilated horizontally by w(dy) = isqrt(r^2 - dy^2):
//                         rows of equal w are ORed first (dilation distributes over OR), each group is dilated once by
//                         shift-and-OR with doubling over the 192-bit window (previous, own, next word).
//
// Bit i of word j of a row is pixel x = 64 j + i; bits at x >= W are zero.  All sums are integer: wave / block sums, then one
// atomicAdd per workgroup and counter (order independent, hence deterministic).  No float atomics.
#include "frtm_common.h"
#include "../../include/frtm_hip.h"
#include <cstdint>

#define JF_IDS 16          // ids per launch of pass 1: 4 counters each = the 64 lanes of a wave
#define JF_ROWS 32         // rows per wave of pass 1
#define JF_MAX_R 64

struct JfIds { int id[JF_IDS]; };

typedef unsigned long long u64;

template <typename L>
__global__ __launch_bounds__(256) void k_jf_planes(const L* __restrict__ pred, const L* __restrict__ truth, int H, int W, int Wd, JfIds ids,
                                                   int k0, int kn, int K, u64* __restrict__ planes, int* __restrict__ counts) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = blockIdx.x * 4 + wv, t = blockIdx.z;
  const int y_begin = blockIdx.y * JF_ROWS, y_end = min(y_begin + JF_ROWS, H);
  int acc = 0;                                               // lane 4 * k + c: counter c of id k (inter, union, n_fg, n_gt)
  if (j < Wd) {
    const int x = j * 64 + lane;
    const bool valid = x < W;
    const int xc = valid ? x : W - 1, xe = min(xc + 1, W - 1);
    const size_t HW = (size_t)H * W, WdH = (size_t)H * Wd;
    const L* p = pred + (size_t)t * HW;
    const L* g = truth + (size_t)t * HW;
    int p0 = (int)p[(size_t)y_begin * W + xc], pe = (int)p[(size_t)y_begin * W + xe];
    int g0 = (int)g[(size_t)y_begin * W + xc], ge = (int)g[(size_t)y_begin * W + xe];
    for (int y = y_begin; y < y_end; ++y) {
      const size_t rs = (size_t)min(y + 1, H - 1) * W;
      const int ps = (int)p[rs + xc], pse = (int)p[rs + xe], gs = (int)g[rs + xc], gse = (int)g[rs + xe];
      for (int k = 0; k < kn; ++k) {
        const int id = ids.id[k];
        const bool f = p0 == id, t0 = g0 == id;
        const bool bf = valid && (f != (pe == id) || f != (ps == id) || f != (pse == id));
        const bool bg = valid && (t0 != (ge == id) || t0 != (gs == id) || t0 != (gse == id));
        const u64 wf = __ballot(bf), wg = __ballot(bg);
        const int c_inter = __popcll(__ballot(valid && f && t0)), c_union = __popcll(__ballot(valid && (f || t0)));
        const int c_fg = __popcll(wf), c_gt = __popcll(wg);
        const int c = lane & 3;
        const int mine = c == 0 ? c_inter : c == 1 ? c_union : c == 2 ? c_fg : c_gt;
        acc += (lane >> 2) == k ? mine : 0;
        if (lane == 0) {
          u64* pl = planes + ((size_t)(t * K + k0 + k) * 2) * WdH + (size_t)y * Wd + j;
          pl[0] = wf;
          pl[WdH] = wg;
        }
      }
      p0 = ps; pe = pse; g0 = gs; ge = gse;
    }
  }
  __shared__ int red[4][64];
  red[wv][lane] = acc;
  __syncthreads();
  if (wv == 0) {
    const int tot = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    if (tot != 0 && (lane >> 2) < kn) atomicAdd(&counts[(size_t)(t * K + k0 + (lane >> 2)) * 6 + (lane & 3)], tot);
  }
}

// y |= y << s over 192 bits (y0 lowest), 1 <= s <= 64
__device__ __forceinline__ void jf_shl_or(u64& y0, u64& y1, u64& y2, int s) {
  if (s == 64) {
    y2 |= y1;
    y1 |= y0;
  } else {
    y2 |= (y2 << s) | (y1 >> (64 - s));
    y1 |= (y1 << s) | (y0 >> (64 - s));
    y0 |= y0 << s;
  }
}

// The middle word of the 192-bit window (a0 previous, a1 own, a2 next word) dilated horizontally by w pixels each way, 0 <= w <= 64.
__device__ __forceinline__ u64 jf_dilate(u64 a0, u64 a1, u64 a2, int w) {
  const int span = 2 * w + 1;                                // y[i] = OR of a[i - s], s = 0 ... 2w; the answer is y[64 + w ... 128 + w)
  int cover = 1;
  while (2 * cover <= span) { jf_shl_or(a0, a1, a2, cover); cover *= 2; }
  if (span > cover) jf_shl_or(a0, a1, a2, span - cover);     // span - cover < cover <= 64
  return w == 0 ? a1 : w == 64 ? a2 : (a1 >> w) | (a2 << (64 - w));
}

__global__ __launch_bounds__(256) void k_jf_match(const u64* __restrict__ planes, int H, int Wd, int r, int* __restrict__ counts) {
  __shared__ int wtab[JF_MAX_R + 2];
  __shared__ int wsum[4];
  if ((int)threadIdx.x <= r) {
    const int d = threadIdx.x, v = r * r - d * d;
    int w = (int)sqrtf((float)v);
    while (w * w > v) --w;
    while ((w + 1) * (w + 1) <= v) ++w;
    wtab[d] = w;
  }
  if ((int)threadIdx.x == r + 1) wtab[r + 1] = -1;           // sentinel: ends the last group
  __syncthreads();
  const int tk = blockIdx.y >> 1, dir = blockIdx.y & 1;     // dir 0: points = pred boundary, of = truth boundary (fg_match); 1: the other way
  const size_t WdH = (size_t)H * Wd;
  const u64* pts = planes + ((size_t)tk * 2 + dir) * WdH;
  const u64* of = planes + ((size_t)tk * 2 + (dir ^ 1)) * WdH;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  int c = 0;
  if (idx < H * Wd) {
    const u64 pw = pts[idx];
    if (pw != 0) {
      const int y = idx / Wd, j = idx - y * Wd;
      const bool has_l = j > 0, has_r = j + 1 < Wd;
      u64 hit = 0;
      int d = 0;
      while (d <= r) {
        const int w = wtab[d];
        u64 a0 = 0, a1 = 0, a2 = 0;
        do {
          const int ya = y - d, yb = y + d;
          if (ya >= 0) {
            const u64* row = of + (size_t)ya * Wd + j;
            a1 |= row[0];
            if (has_l) a0 |= row[-1];
            if (has_r) a2 |= row[1];
          }
          if (d > 0 && yb < H) {
            const u64* row = of + (size_t)yb * Wd + j;
            a1 |= row[0];
            if (has_l) a0 |= row[-1];
            if (has_r) a2 |= row[1];
          }
          ++d;
        } while (wtab[d] == w);
        if ((a0 | a1 | a2) != 0) hit |= jf_dilate(a0, a1, a2, w);
      }
      c = __popcll(pw & hit);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    if (tot) atomicAdd(&counts[(size_t)tk * 6 + 4 + dir], tot);
  }
}

extern "C" {

size_t frtm_jf_workspace_bytes(int T, int H, int W, int K) {
  if (T < 1 || H < 1 || W < 1 || K < 1) return 0;
  return (size_t)T * K * 2 * H * (size_t)((W + 63) / 64) * sizeof(u64);
}

int frtm_jf_counts(const void* pred, const void* truth, int label_bytes, int T, int H, int W, const int* ids, int K, int r, int* counts,
                   void* ws, size_t ws_bytes, frtm_stream_t stream) {
  FRTM_CHECK_ARG(pred && truth && ids && counts && ws, "frtm_jf_counts: null argument");
  FRTM_CHECK_ARG(label_bytes == 1 || label_bytes == 4, "frtm_jf_counts: label_bytes must be 1 (uint8) or 4 (int32), got %d", label_bytes);
  FRTM_CHECK_ARG(T >= 1 && H >= 1 && W >= 1 && K >= 1, "frtm_jf_counts: T, H, W, K must be >= 1 (got %d, %d, %d, %d)", T, H, W, K);
  FRTM_CHECK_ARG((long long)H * W < (1LL << 31), "frtm_jf_counts: H * W must be below 2^31 (got %d x %d)", H, W);
  FRTM_CHECK_ARG(r >= 1 && r <= JF_MAX_R, "frtm_jf_counts: disk radius %d outside 1 ... %d", r, JF_MAX_R);
  FRTM_CHECK_ARG((long long)T * K * 2 <= 65535 && T <= 65535 && (long long)T * K * 6 < (1LL << 31),
                 "frtm_jf_counts: T * K = %d * %d too large for one call (T * K * 2 <= 65535): split the frames", T, K);
  FRTM_CHECK_ARG(ws_bytes >= frtm_jf_workspace_bytes(T, H, W, K), "frtm_jf_counts: workspace of %zu bytes, need %zu", ws_bytes,
                 frtm_jf_workspace_bytes(T, H, W, K));
  hipStream_t st = (hipStream_t)stream;
  const int Wd = (W + 63) / 64;
  FRTM_CHECK_ARG(ceil_div(H, JF_ROWS) <= 65535, "frtm_jf_counts: H = %d too large", H);
  FRTM_HIP(hipMemsetAsync(counts, 0, sizeof(int) * (size_t)T * K * 6, st));
  dim3 g1(ceil_div(Wd, 4), ceil_div(H, JF_ROWS), T);
  for (int k0 = 0; k0 < K; k0 += JF_IDS) {
    JfIds s;
    const int kn = min(JF_IDS, K - k0);
    for (int k = 0; k < JF_IDS; ++k) s.id[k] = k < kn ? ids[k0 + k] : 0;
    if (label_bytes == 1)
      k_jf_planes<unsigned char><<<g1, 256, 0, st>>>((const unsigned char*)pred, (const unsigned char*)truth, H, W, Wd, s, k0, kn, K, (u64*)ws, counts);
    else
      k_jf_planes<int><<<g1, 256, 0, st>>>((const int*)pred, (const int*)truth, H, W, Wd, s, k0, kn, K, (u64*)ws, counts);
    FRTM_LAUNCH_CHECK();
  }
  dim3 g2(ceil_div(H * Wd, 256), T * K * 2);
  k_jf_match<<<g2, 256, 0, st>>>((const u64*)ws, H, Wd, r, counts);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

}  // extern "C"
