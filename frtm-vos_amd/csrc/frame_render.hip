// The way out: tracked objects rendered onto their frames -- planar RGB or NV12 surfaces, any sizes -- for all frames of a tick in ONE launch
// (ops.render_frames, Tracker.render, StreamPool.render).  The answer of a frame is a uint8 label map or a merged fp32 mask stack with its
// LUT (decoded by native_size.hip's rule, per_frame.h); the style is a 256-row table (c0, c1, c2, a) indexed by object id, in the frame's
// own channels: R,G,B for planar RGB, Y,U,V for NV12 (the host converts the palette; the kernel knows no colour matrix).
//
// Every output byte is an integer function of the inputs (include/frtm_hip.h has the full statement):
//   s = the pixel's three channel bytes; NV12: Y and the chroma sample of its 2 x 2 block, replicated like frtm_frames_to_rgb_u8's
//   mix(s, c, a) = (t + (t >> 8)) >> 8,  t = s (255 - a) + c a + 128               ( = round(s + (c - s) a / 255), half up )
//   hard:  out = mix(s, c_id, a_id);  with edge_alpha, a pixel of an object with a 4-neighbour of another label inside the picture takes edge_alpha
//   soft:  m = clamp(m_k*, 0, 1), k* the first k >= 1 with the largest m_k;  B = mix(s, c_b, a_b), F = mix(s, c_f, a_f), b = lut[0], f = lut[k*]
//          out = (int)rintf(fmaf(m, F - B, B))
//   NV12:  Y' per pixel; U', V' = (sum of the block's per-pixel results + cnt / 2) / cnt over the cnt = 1, 2 or 4 pixels the picture has there
// Loads and stores touch picture samples only, in the source and in the destination; the destination may be the source itself.
#include "frtm_common.h"
#include "per_frame.h"       // MERGE_MAX, merged_offer, merged_plane
#include "../../include/frtm_hip.h"
#include <cstdint>

#define RN_TH 16            // tile: rows (thread (tx, tg) owns rows tg + 4 i); the origin is even, so no chroma block straddles two tiles
#define RN_TW 64            //       columns: lane = column, so a wave stores 64 consecutive bytes
#define RN_LP 68            // bytes per LDS row of the label patch (RN_TW + 2 halo columns, padded)
#define RN_MAXDIM 16384
#define RN_MAXBYTES (1LL << 46)   // no buffer is larger: pitch * h then stays below 2^60
#define RN_ROW FRTM_RENDER_ROW_WORDS

// words of a table row
enum { RW_FORMAT, RW_H, RW_W, RW_SRC, RW_SRC_BYTES, RW_SRC_PITCH, RW_SRC_UV, RW_DST, RW_DST_BYTES, RW_DST_PITCH, RW_DST_UV, RW_FORM, RW_ANS,
       RW_ANS_BYTES, RW_K, RW_LUT, RW_STYLE, RW_SOFT, RW_EDGE, RW_ZERO };
// why a row is refused
enum { RN_OK, RN_BAD_ENUM, RN_BAD_SIZE, RN_NULL, RN_BAD_K, RN_BAD_FLAGS, RN_SOFT_LABELS, RN_NOT_A_SIZE, RN_SRC_PITCH, RN_DST_PITCH, RN_SRC_RANGE,
       RN_DST_RANGE, RN_ANS_RANGE, RN_ANS_ALIGN, RN_OVERLAP, RN_ANS_OVERLAP };

// Bytes from a surface's first sample to the end of its last row (DecoderFrame.layout's nbytes_needed), or -1 (pitch) / -2 (range).
__host__ __device__ static inline long long rn_span(long long format, long long h, long long w, long long pitch, long long uv_off, long long bytes) {
  if (format == FRTM_RENDER_RGB) return 3 * h * w;
  if (pitch < 2 * ((w + 1) / 2)) return -1;
  if (pitch > bytes || uv_off < pitch * h || uv_off > bytes) return -2;
  return uv_off + pitch * ((h + 1) / 2);
}

// Is row r a frame this launch can render?  (Evaluated by the host from its copy, for the messages and the grid, and by every workgroup from
// the DEVICE table before it touches anything: a device table that differs from the checked one reads and writes nothing out of bounds.)
__host__ __device__ static inline int rn_check(const long long* r) {
  const long long format = r[RW_FORMAT], h = r[RW_H], w = r[RW_W], form = r[RW_FORM], K = r[RW_K];
  if ((format != FRTM_RENDER_RGB && format != FRTM_RENDER_NV12) || (form != FRTM_RENDER_LABELS && form != FRTM_RENDER_MASKS) || r[RW_ZERO] != 0)
    return RN_BAD_ENUM;
  if (h < 1 || w < 1 || h > RN_MAXDIM || w > RN_MAXDIM) return RN_BAD_SIZE;
  if (form == FRTM_RENDER_MASKS && (K < 1 || K > MERGE_MAX)) return RN_BAD_K;
  if (!r[RW_SRC] || !r[RW_DST] || !r[RW_ANS] || !r[RW_STYLE] || (form == FRTM_RENDER_MASKS && !r[RW_LUT])) return RN_NULL;
  if ((r[RW_SOFT] != 0 && r[RW_SOFT] != 1) || r[RW_EDGE] < -1 || r[RW_EDGE] > 255 || (r[RW_SOFT] == 1 && r[RW_EDGE] != -1)) return RN_BAD_FLAGS;
  if (r[RW_SOFT] == 1 && form == FRTM_RENDER_LABELS) return RN_SOFT_LABELS;
  const long long sb = r[RW_SRC_BYTES], db = r[RW_DST_BYTES], ab = r[RW_ANS_BYTES];
  if (sb < 0 || db < 0 || ab < 0 || sb > RN_MAXBYTES || db > RN_MAXBYTES || ab > RN_MAXBYTES) return RN_NOT_A_SIZE;
  const long long ss = rn_span(format, h, w, r[RW_SRC_PITCH], r[RW_SRC_UV], sb), ds = rn_span(format, h, w, r[RW_DST_PITCH], r[RW_DST_UV], db);
  if (ss == -1) return RN_SRC_PITCH;
  if (ds == -1) return RN_DST_PITCH;
  if (ss < 0 || ss > sb) return RN_SRC_RANGE;
  if (ds < 0 || ds > db) return RN_DST_RANGE;
  const long long as = form == FRTM_RENDER_MASKS ? 4 * K * h * w : h * w;
  if (as > ab) return RN_ANS_RANGE;
  if (form == FRTM_RENDER_MASKS && (r[RW_ANS] & 3)) return RN_ANS_ALIGN;
  // the destination is the source itself, sample for sample, or shares no byte with it; and it shares none with the answer
  const unsigned long long s0 = (unsigned long long)r[RW_SRC], d0 = (unsigned long long)r[RW_DST], a0 = (unsigned long long)r[RW_ANS];
  const bool in_place = s0 == d0 && (format == FRTM_RENDER_RGB || (r[RW_SRC_PITCH] == r[RW_DST_PITCH] && r[RW_SRC_UV] == r[RW_DST_UV]));
  if (!in_place && s0 < d0 + (unsigned long long)ds && d0 < s0 + (unsigned long long)ss) return RN_OVERLAP;
  if (a0 < d0 + (unsigned long long)ds && d0 < a0 + (unsigned long long)as) return RN_ANS_OVERLAP;
  return RN_OK;
}

__device__ __forceinline__ int rn_mix(int s, int c, int a) {
  const int t = s * (255 - a) + c * a + 128;
  return (t + (t >> 8)) >> 8;
}

// One workgroup = one RN_TH x RN_TW tile of one frame (blockIdx.z).  (1) the tile's labels with a 1-pixel halo -- or, soft, its m and
// foreground id -- into LDS, the style table beside them; (2) every thread loads the samples of its four pixels and computes their bytes,
// the per-pixel chroma results of an NV12 frame go to LDS; (3) after the barrier -- every load of the tile has been consumed, so an in-place
// frame loses nothing -- the stores: four Y (or 3 x 4 R,G,B) bytes per thread, and one of the tile's 8 x 32 chroma samples per thread.
__global__ __launch_bounds__(256) void k_render_frames(const long long* __restrict__ table) {
  __shared__ unsigned char lab[(RN_TH + 2) * RN_LP];
  __shared__ float msoft[RN_TH * RN_TW];
  __shared__ unsigned char fid[RN_TH * RN_TW];
  __shared__ unsigned char uvp[RN_TH * RN_TW * 2];
  __shared__ uchar4 sty[256];
  const long long* row = table + (size_t)RN_ROW * blockIdx.z;
  if (rn_check(row) != RN_OK) return;                                    // (uniform per workgroup, before any barrier)
  const int h = (int)row[RW_H], w = (int)row[RW_W];
  const int y0 = blockIdx.y * RN_TH, x0 = blockIdx.x * RN_TW;
  if (y0 >= h || x0 >= w) return;                                       // (the grid is sized for the launch's largest frame)
  const bool nv12 = row[RW_FORMAT] == FRTM_RENDER_NV12, stack = row[RW_FORM] == FRTM_RENDER_MASKS, soft = row[RW_SOFT] == 1;
  const int K = stack ? (int)row[RW_K] : 0, edge = (int)row[RW_EDGE];
  const unsigned char* src = (const unsigned char*)row[RW_SRC];         // (no __restrict__: the destination may be the source)
  unsigned char* dst = (unsigned char*)row[RW_DST];
  const unsigned char* ans8 = (const unsigned char*)row[RW_ANS];
  const float* ansf = (const float*)row[RW_ANS];
  const unsigned char* lut = (const unsigned char*)row[RW_LUT];
  const unsigned char* style = (const unsigned char*)row[RW_STYLE];
  const size_t hw = (size_t)h * w;
  const int tid = threadIdx.x, tx = tid & 63, tg = tid >> 6;

  sty[tid] = make_uchar4(style[4 * tid], style[4 * tid + 1], style[4 * tid + 2], style[4 * tid + 3]);
  const int bg = stack ? lut[0] : 0;
  if (!soft) {
    // cell (r, c) = the label of pixel (y0 - 1 + r, x0 - 1 + c), coordinates clamped into the picture: a neighbour beyond the picture's
    // border is the pixel itself, so the border makes no edge
    for (int i = tid; i < (RN_TH + 2) * (RN_TW + 2); i += 256) {
      const int r = i / (RN_TW + 2), c = i - r * (RN_TW + 2);
      const int y = min(max(y0 - 1 + r, 0), h - 1), x = min(max(x0 - 1 + c, 0), w - 1);
      const size_t pix = (size_t)y * w + x;
      int id;
      if (stack) {
        float best = -INFINITY; int arg = 0;
        for (int k = 0; k < K; ++k) merged_offer(ansf[k * hw + pix], k, best, arg);
        id = lut[merged_plane(arg, best)];
      } else {
        id = ans8[pix];
      }
      lab[r * RN_LP + c] = (unsigned char)id;
    }
  } else {
    for (int i = tid; i < RN_TH * RN_TW; i += 256) {
      const int y = min(y0 + (i >> 6), h - 1), x = min(x0 + (i & 63), w - 1);
      const size_t pix = (size_t)y * w + x;
      float best = -INFINITY; int ks = 1;                                // no plane above -inf (K = 1, or NaNs only): m = 0
      for (int k = 1; k < K; ++k) merged_offer(ansf[k * hw + pix], k, best, ks);
      msoft[i] = fminf(fmaxf(best, 0.f), 1.f);
      fid[i] = K > 1 ? lut[ks] : (unsigned char)bg;
    }
  }
  __syncthreads();

  const long long spitch = row[RW_SRC_PITCH], dpitch = row[RW_DST_PITCH];
  const unsigned char* suv = src + row[RW_SRC_UV];
  unsigned char* duv = dst + row[RW_DST_UV];
  const int x = x0 + tx;
  int o[4][3];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ly = tg + 4 * i, y = y0 + ly;
    o[i][0] = o[i][1] = o[i][2] = 0;
    if (y >= h || x >= w) continue;
    int s[3];
    if (nv12) {
      const unsigned char* uv = suv + (size_t)(y >> 1) * spitch + 2 * (x >> 1);
      s[0] = src[(size_t)y * spitch + x]; s[1] = uv[0]; s[2] = uv[1];
    } else {
      const size_t pix = (size_t)y * w + x;
      s[0] = src[pix]; s[1] = src[hw + pix]; s[2] = src[2 * hw + pix];
    }
    if (!soft) {
      const unsigned char* p = lab + (ly + 1) * RN_LP + tx + 1;
      const int id = p[0];
      const uchar4 st = sty[id];
      int a = st.w;
      if (edge >= 0 && id != bg && (p[-RN_LP] != id || p[RN_LP] != id || p[-1] != id || p[1] != id)) a = edge;
      o[i][0] = rn_mix(s[0], st.x, a); o[i][1] = rn_mix(s[1], st.y, a); o[i][2] = rn_mix(s[2], st.z, a);
    } else {
      const float m = msoft[ly * RN_TW + tx];
      const uchar4 sb = sty[bg], sf = sty[fid[ly * RN_TW + tx]];
      const int cb[3] = {sb.x, sb.y, sb.z}, cf[3] = {sf.x, sf.y, sf.z};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int B = rn_mix(s[c], cb[c], sb.w), F = rn_mix(s[c], cf[c], sf.w);
        o[i][c] = (int)rintf(__fmaf_rn(m, (float)(F - B), (float)B));
      }
    }
    if (nv12) { uvp[2 * (ly * RN_TW + tx)] = (unsigned char)o[i][1]; uvp[2 * (ly * RN_TW + tx) + 1] = (unsigned char)o[i][2]; }
  }
  __syncthreads();

#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int y = y0 + tg + 4 * i;
    if (y >= h || x >= w) continue;
    if (nv12) {
      dst[(size_t)y * dpitch + x] = (unsigned char)o[i][0];
    } else {
      const size_t pix = (size_t)y * w + x;
      dst[pix] = (unsigned char)o[i][0]; dst[hw + pix] = (unsigned char)o[i][1]; dst[2 * hw + pix] = (unsigned char)o[i][2];
    }
  }
  if (nv12) {
    const int cj = tid >> 5, ci = tid & 31;                              // chroma sample (y0 / 2 + cj, x0 / 2 + ci) covers tile rows 2 cj, 2 cj + 1
    const int ry = y0 + 2 * cj, rx = x0 + 2 * ci;
    if (ry < h && rx < w) {
      const int nr = min(2, h - ry), nc = min(2, w - rx);
      int su = 0, sv = 0;
      for (int a = 0; a < nr; ++a)
        for (int b = 0; b < nc; ++b) {
          const unsigned char* q = uvp + 2 * ((2 * cj + a) * RN_TW + 2 * ci + b);
          su += q[0]; sv += q[1];
        }
      const int cnt = nr * nc, sh = cnt == 4 ? 2 : cnt == 2 ? 1 : 0;    // cnt is 1, 2 or 4
      const int U = (su + (cnt >> 1)) >> sh, V = (sv + (cnt >> 1)) >> sh;
      unsigned char* q = duv + (size_t)(ry >> 1) * dpitch + rx;         // (2 * (rx >> 1) = rx: rx is even)
      if (((uintptr_t)q & 1) == 0) {
        *(unsigned short*)q = (unsigned short)(U | (V << 8));          // one 2-byte store where the sample is aligned
      } else {
        q[0] = (unsigned char)U; q[1] = (unsigned char)V;
      }
    }
  }
}

extern "C" int frtm_render_frames_u8(const long long* table_host, const long long* table_dev, int n, frtm_stream_t stream) {
  const char* who = "frtm_render_frames_u8";
  FRTM_CHECK_ARG(table_host && table_dev, "%s: bad argument (a null table)", who);
  FRTM_CHECK_ARG(n >= 1 && n <= 65535, "%s: n = %d frames (1 .. 65535)", who, n);
  int maxH = 0, maxW = 0;
  for (int i = 0; i < n; ++i) {
    const long long* r = table_host + (size_t)RN_ROW * i;
    const int why = rn_check(r);
    const long long chroma_row = 2 * ((r[RW_W] + 1) / 2);
    switch (why) {
      case RN_OK: break;
      case RN_BAD_ENUM:
        FRTM_CHECK_ARG(false, "%s: frame %d has format %lld, answer form %lld and last word %lld (a format and a form of include/frtm_hip.h, and 0)", who,
                       i, r[RW_FORMAT], r[RW_FORM], r[RW_ZERO]);
      case RN_BAD_SIZE: FRTM_CHECK_ARG(false, "%s: frame %d has size %lld x %lld (1 .. %d)", who, i, r[RW_H], r[RW_W], RN_MAXDIM);
      case RN_BAD_K: FRTM_CHECK_ARG(false, "%s: frame %d has a stack of %lld planes (1 .. %d)", who, i, r[RW_K], MERGE_MAX);
      case RN_NULL: FRTM_CHECK_ARG(false, "%s: frame %d has a null address (source, destination, answer, style or LUT)", who, i);
      case RN_BAD_FLAGS:
        FRTM_CHECK_ARG(false, "%s: frame %d has soft %lld and edge_alpha %lld (0 or 1; -1 .. 255; no edge under soft)", who, i, r[RW_SOFT], r[RW_EDGE]);
      case RN_SOFT_LABELS: FRTM_CHECK_ARG(false, "%s: frame %d asks for a soft blend of a label map (soft needs a mask stack)", who, i);
      case RN_NOT_A_SIZE: FRTM_CHECK_ARG(false, "%s: frame %d: a buffer size is not a size", who, i);
      case RN_SRC_PITCH: FRTM_CHECK_ARG(false, "%s: frame %d has source pitch %lld, below its %lld-byte chroma row", who, i, r[RW_SRC_PITCH], chroma_row);
      case RN_DST_PITCH:
        FRTM_CHECK_ARG(false, "%s: frame %d has destination pitch %lld, below its %lld-byte chroma row", who, i, r[RW_DST_PITCH], chroma_row);
      case RN_SRC_RANGE:
        FRTM_CHECK_ARG(false, "%s: frame %d's source (%lld x %lld, pitch %lld, chroma at %lld) leaves its %lld-byte buffer", who, i, r[RW_H], r[RW_W],
                       r[RW_SRC_PITCH], r[RW_SRC_UV], r[RW_SRC_BYTES]);
      case RN_DST_RANGE:
        FRTM_CHECK_ARG(false, "%s: frame %d's destination (%lld x %lld, pitch %lld, chroma at %lld) leaves its %lld-byte buffer", who, i, r[RW_H], r[RW_W],
                       r[RW_DST_PITCH], r[RW_DST_UV], r[RW_DST_BYTES]);
      case RN_ANS_RANGE: FRTM_CHECK_ARG(false, "%s: frame %d's answer leaves its %lld-byte buffer", who, i, r[RW_ANS_BYTES]);
      case RN_ANS_ALIGN: FRTM_CHECK_ARG(false, "%s: frame %d's mask stack is not 4-byte aligned", who, i);
      case RN_OVERLAP:
        FRTM_CHECK_ARG(false, "%s: frame %d's destination overlaps its source in part (in place means the same address and layout)", who, i);
      default: FRTM_CHECK_ARG(false, "%s: frame %d's destination overlaps its answer", who, i);
    }
    maxH = max(maxH, (int)r[RW_H]);
    maxW = max(maxW, (int)r[RW_W]);
  }
  dim3 g(ceil_div(maxW, RN_TW), ceil_div(maxH, RN_TH), n);
  k_render_frames<<<g, 256, 0, (hipStream_t)stream>>>(table_dev);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}
