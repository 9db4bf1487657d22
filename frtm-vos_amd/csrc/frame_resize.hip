// Batched resize of native-size training frames and label maps to the training size (lib/training_datasets.py: DeviceFrameResizer).
// Counterpart of what the reference does per frame on the CPU in lib/training_datasets.py:185-195: cv2.resize(im, (854, 480), INTER_AREA or
// INTER_CUBIC) and F.interpolate((lb == obj_id), (480, 854), mode='nearest').  OpenCV is not available here; the operators are restated:
//
//   area   separable.  An axis with src > dst: output d is the mean of the source interval [d s, (d + 1) s), s = src / dst, edge pixels
//          with their fractional coverage.  src == dst: the identity (the same formula: one tap of weight 1).  src < dst: bilinear with
//          half-pixel centres and a replicate border (a deviation from OpenCV's INTER_AREA, which enlarges differently: DESIGN.md section 7).
//   cubic  frtm_bicubic_resize's operator (A = -0.75, half-pixel centres, replicate border, any ratio) on uint8.
//   label  (src == obj_id) at F.interpolate(mode='nearest')'s source index min(floor(dst * float(src) / dst_size), src - 1), the product
//          in float32 as torch forms it.
//
// Tap positions and the quantities the weights are made of are INTEGERS (an interval end d * src in units of 1 / dst pixel; the
// sub-pixel phase ((2 d + 1) src - dst) mod 2 dst), so every weight is one correctly rounded fp32 division away from its exact value and
// the weights of an integer ratio are exact.  Sums are fp32; one rounding to nearest-even and a clamp to 0..255 at the end.
#include "frtm_common.h"
#include "../../include/frtm_hip.h"
#include <cstdint>

#define FR_TH 16            // output tile: rows
#define FR_TW 64            //              columns (one wave per row group: lane = column)
#define FR_PR 32            // source rows per staged chunk
#define FR_PC 240           // source columns per staged chunk
#define FR_WORDS 16         // 16-byte words per LDS patch row: FR_PC bytes plus the up to 15 bytes in front of an unaligned row start
#define FR_PCB (16 * FR_WORDS)
#define FR_MAXDIM 16384     // (2 d + 1) * src and (s + 1) * dst stay below 2^31

enum { AX_AREA = 0, AX_LINEAR = 1, AX_CUBIC = 2 };
struct Axis { int kind, src, dst; };

__device__ __forceinline__ Axis make_axis(int mode, int src, int dst) {
  Axis a;
  a.kind = mode == FRTM_RESIZE_CUBIC ? AX_CUBIC : (src >= dst ? AX_AREA : AX_LINEAR);
  a.src = src;
  a.dst = dst;
  return a;
}

// Output index d reads the source indices first .. first + n - 1 (not yet clamped into the map; only the interpolating kinds leave it).
// rem: the sub-pixel phase of the interpolating kinds in units of 1 / (2 dst).
__device__ __forceinline__ void axis_span(const Axis a, int d, int& first, int& n, int& rem) {
  if (a.kind == AX_AREA) {
    first = d * a.src / a.dst;
    n = ((d + 1) * a.src - 1) / a.dst - first + 1;
    rem = 0;
    return;
  }
  const int num = (2 * d + 1) * a.src - a.dst, den = 2 * a.dst;       // source coordinate (d + 0.5) src / dst - 0.5 = num / den > -1
  const int fl = num >= 0 ? num / den : -1;
  rem = num - fl * den;
  first = a.kind == AX_LINEAR ? fl : fl - 1;
  n = a.kind == AX_LINEAR ? 2 : 4;
}

__device__ __forceinline__ float axis_weight(const Axis a, int d, int first, int rem, int j) {
  if (a.kind == AX_AREA) {
    const int s = first + j;
    const int lo = max(s * a.dst, d * a.src), hi = min((s + 1) * a.dst, (d + 1) * a.src);
    return __fdiv_rn((float)(hi - lo), (float)a.src);
  }
  const int den = 2 * a.dst;
  if (a.kind == AX_LINEAR) return __fdiv_rn((float)(j ? rem : den - rem), (float)den);
  const float A = -0.75f, t = __fdiv_rn((float)rem, (float)den);
  const float x = j == 0 ? t + 1.f : j == 1 ? t : j == 2 ? 1.f - t : 2.f - t;
  return (j == 0 || j == 3) ? ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A : ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
}

// One workgroup = one FR_TH x FR_TW output tile of one plane of one frame.  The tile's source footprint is walked in chunks of FR_PR rows x
// FR_PC columns (a 1.5x reduction fits one chunk; a larger ratio loops): the chunk's bytes are staged in LDS with 16-byte loads from
// 16-byte aligned ADDRESSES -- a row of a packed frame starts anywhere, so each LDS row keeps its own phase (address & 15) and the words that
// straddle the frame's first or last byte are read byte by byte -- then the horizontal pass leaves one fp32 value per (chunk row, output
// column) and the vertical pass adds the chunk's share to the four outputs a thread owns.
__global__ __launch_bounds__(256) void k_resize_frames(const unsigned char* __restrict__ src, const long long* __restrict__ desc, int planes,
                                                        unsigned char* __restrict__ out, int H, int W) {
  __shared__ __attribute__((aligned(16))) unsigned char patch[FR_PR * FR_PCB];
  __shared__ float hrow[FR_PR * FR_TW];
  const int f = blockIdx.z / planes, pl = blockIdx.z - f * planes;
  const int h = (int)desc[4 * f + 1], w = (int)desc[4 * f + 2], mode = (int)desc[4 * f + 3];
  const unsigned char* fsrc = src + desc[4 * f];                       // the frame: planes * h * w bytes
  const unsigned char* fend = fsrc + (size_t)planes * h * w;
  const unsigned char* psrc = fsrc + (size_t)pl * h * w;
  const Axis ay = make_axis(mode, h, H), ax = make_axis(mode, w, W);
  const int y0 = blockIdx.y * FR_TH, x0 = blockIdx.x * FR_TW;
  const int th = min(FR_TH, H - y0), tw = min(FR_TW, W - x0);
  const int tx = threadIdx.x & 63, tg = threadIdx.x >> 6;
  const bool col_ok = tx < tw;
  const int xo = x0 + min(tx, tw - 1);

  int first, n, rem;
  axis_span(ay, y0, first, n, rem);
  const int R0 = min(max(first, 0), h - 1);
  axis_span(ay, y0 + th - 1, first, n, rem);
  const int R1 = min(max(first + n - 1, 0), h - 1);
  axis_span(ax, x0, first, n, rem);
  const int C0 = min(max(first, 0), w - 1);
  axis_span(ax, x0 + tw - 1, first, n, rem);
  const int C1 = min(max(first + n - 1, 0), w - 1);

  int cf, cn, crem;                                                    // this lane's column taps
  axis_span(ax, xo, cf, cn, crem);
  int rf[4], rn[4], rrem[4];                                           // row taps of the outputs (tg + 4 i, tx) this thread owns
  float acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    axis_span(ay, y0 + min(tg + 4 * i, th - 1), rf[i], rn[i], rrem[i]);
    acc[i] = 0.f;
  }

  for (int rc0 = R0; rc0 <= R1; rc0 += FR_PR) {
    const int rcn = min(FR_PR, R1 - rc0 + 1);
    float hp[FR_PR / 4];                                               // chunk rows tg + 4 i at column tx
#pragma unroll
    for (int i = 0; i < FR_PR / 4; ++i) hp[i] = 0.f;
    for (int cc0 = C0; cc0 <= C1; cc0 += FR_PC) {
      const int ccn = min(FR_PC, C1 - cc0 + 1);
      __syncthreads();                                                 // the previous chunk's readers are done with patch / hrow
      for (int it = threadIdx.x; it < rcn * FR_WORDS; it += 256) {
        const int r = it / FR_WORDS, wi = it - r * FR_WORDS;
        const uintptr_t g = (uintptr_t)(psrc + (size_t)(rc0 + r) * w + cc0);
        const uintptr_t wa = (g & ~(uintptr_t)15) + 16 * wi;           // aligned address of this word; word 0 holds the row's first byte
        if (wa >= g + ccn) continue;
        unsigned char* lds = patch + r * FR_PCB + 16 * wi;
        if (wa >= (uintptr_t)fsrc && wa + 16 <= (uintptr_t)fend) {
          *reinterpret_cast<uint4*>(lds) = *reinterpret_cast<const uint4*>(psrc + (ptrdiff_t)(wa - (uintptr_t)psrc));
        } else {
          for (int b = 0; b < 16; ++b) {
            const uintptr_t p = wa + b;
            lds[b] = (p >= (uintptr_t)fsrc && p < (uintptr_t)fend) ? psrc[(ptrdiff_t)(p - (uintptr_t)psrc)] : (unsigned char)0;
          }
        }
      }
      __syncthreads();
      int lb[FR_PR / 4];                                               // LDS offset of source column 0 in this thread's rows
#pragma unroll
      for (int i = 0; i < FR_PR / 4; ++i) {
        const int r = tg + 4 * i;
        lb[i] = r * FR_PCB + (int)((uintptr_t)(psrc + (size_t)(rc0 + r) * w + cc0) & 15) - cc0;
      }
      const int jb = ax.kind == AX_AREA ? max(0, cc0 - cf) : 0, je = ax.kind == AX_AREA ? min(cn, cc0 + ccn - cf) : cn;
      for (int j = jb; j < je; ++j) {
        const int cs = min(max(cf + j, 0), w - 1);
        if (cs < cc0 || cs >= cc0 + ccn) continue;
        const float wgt = axis_weight(ax, xo, cf, crem, j);
#pragma unroll
        for (int i = 0; i < FR_PR / 4; ++i)
          if (tg + 4 * i < rcn) hp[i] += wgt * (float)patch[lb[i] + cs];
      }
    }
#pragma unroll
    for (int i = 0; i < FR_PR / 4; ++i) hrow[(tg + 4 * i) * FR_TW + tx] = hp[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!col_ok || tg + 4 * i >= th) continue;
      const int jb = ay.kind == AX_AREA ? max(0, rc0 - rf[i]) : 0, je = ay.kind == AX_AREA ? min(rn[i], rc0 + rcn - rf[i]) : rn[i];
      for (int j = jb; j < je; ++j) {
        const int rs = min(max(rf[i] + j, 0), h - 1);
        if (rs < rc0 || rs >= rc0 + rcn) continue;
        acc[i] += axis_weight(ay, y0 + tg + 4 * i, rf[i], rrem[i], j) * hrow[(rs - rc0) * FR_TW + tx];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int y = y0 + tg + 4 * i;
    if (col_ok && tg + 4 * i < th) out[((size_t)blockIdx.z * H + y) * W + xo] = (unsigned char)fminf(fmaxf(rintf(acc[i]), 0.f), 255.f);
  }
}

// Nearest-neighbour gather: every source byte is read at most once when reducing and a few times from L1 when enlarging, so there is no
// footprint worth staging.  blockIdx.y = frame.
__global__ __launch_bounds__(256) void k_resize_labels(const unsigned char* __restrict__ src, const long long* __restrict__ desc,
                                                        unsigned char* __restrict__ out, int H, int W) {
  const int f = blockIdx.y;
  const int h = (int)desc[4 * f + 1], w = (int)desc[4 * f + 2];
  const unsigned char id = (unsigned char)desc[4 * f + 3];
  const unsigned char* s = src + desc[4 * f];
  const float sy = __fdiv_rn((float)h, (float)H), sx = __fdiv_rn((float)w, (float)W);
  const int total = H * W;
  for (int pix = blockIdx.x * 256 + threadIdx.x; pix < total; pix += gridDim.x * 256) {
    const int y = pix / W, x = pix - y * W;
    const int ys = min((int)floorf(__fmul_rn((float)y, sy)), h - 1), xs = min((int)floorf(__fmul_rn((float)x, sx)), w - 1);
    out[(size_t)f * total + pix] = s[(size_t)ys * w + xs] == id ? 1 : 0;
  }
}

// rows of the host table: {byte offset, h, w, last}; the frame's bytes must lie inside [0, src_bytes)
static int check_table(const char* who, const long long* d, int n, size_t planes, size_t src_bytes, long long last_lo, long long last_hi) {
  for (int i = 0; i < n; ++i) {
    const long long off = d[4 * i], h = d[4 * i + 1], w = d[4 * i + 2], last = d[4 * i + 3];
    FRTM_CHECK_ARG(h >= 1 && w >= 1 && h <= FR_MAXDIM && w <= FR_MAXDIM, "%s: frame %d has size %lld x %lld (1 .. %d)", who, i, h, w, FR_MAXDIM);
    FRTM_CHECK_ARG(last >= last_lo && last <= last_hi, "%s: frame %d has mode / object id %lld (%lld .. %lld)", who, i, last, last_lo, last_hi);
    FRTM_CHECK_ARG(off >= 0 && (size_t)off <= src_bytes && planes * (size_t)h * (size_t)w <= src_bytes - (size_t)off,
                   "%s: frame %d (offset %lld, %zu x %lld x %lld bytes) leaves the %zu-byte source buffer", who, i, off, planes, h, w, src_bytes);
  }
  return FRTM_OK;
}

extern "C" int frtm_resize_frames_u8(const unsigned char* src, size_t src_bytes, const long long* desc_host, const long long* desc_dev, int n,
                                     int planes, unsigned char* out, int H, int W, frtm_stream_t stream) {
  FRTM_CHECK_ARG(src && desc_host && desc_dev && out && n >= 1 && planes >= 1, "frtm_resize_frames_u8: bad argument");
  FRTM_CHECK_ARG(H >= 1 && W >= 1 && H <= FR_MAXDIM && W <= FR_MAXDIM, "frtm_resize_frames_u8: output size %d x %d (1 .. %d)", H, W, FR_MAXDIM);
  FRTM_CHECK_ARG((long long)n * planes <= 65535, "frtm_resize_frames_u8: at most 65535 planes per call");
  if (int rc = check_table("frtm_resize_frames_u8", desc_host, n, (size_t)planes, src_bytes, FRTM_RESIZE_AREA, FRTM_RESIZE_CUBIC)) return rc;
  dim3 g(ceil_div(W, FR_TW), ceil_div(H, FR_TH), n * planes);
  k_resize_frames<<<g, 256, 0, (hipStream_t)stream>>>(src, desc_dev, planes, out, H, W);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

extern "C" int frtm_resize_labels_u8(const unsigned char* src, size_t src_bytes, const long long* desc_host, const long long* desc_dev, int n,
                                     unsigned char* out, int H, int W, frtm_stream_t stream) {
  FRTM_CHECK_ARG(src && desc_host && desc_dev && out && n >= 1 && n <= 65535, "frtm_resize_labels_u8: bad argument");
  FRTM_CHECK_ARG(H >= 1 && W >= 1 && H <= FR_MAXDIM && W <= FR_MAXDIM, "frtm_resize_labels_u8: output size %d x %d (1 .. %d)", H, W, FR_MAXDIM);
  if (int rc = check_table("frtm_resize_labels_u8", desc_host, n, 1, src_bytes, 0, 255)) return rc;
  dim3 g((unsigned)min(ceil_div(H * W, 256), 1024), n);
  k_resize_labels<<<g, 256, 0, (hipStream_t)stream>>>(src, desc_dev, out, H, W);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}
