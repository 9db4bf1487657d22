// The way back from the working size (Tracker(working_size=...), StreamPool(working_size=...)): native-size label maps and masks from
// the merged mask stacks at the working size, for all frames of a tick in ONE launch whatever their native sizes and object counts; and
// the id-preserving nearest resize of a first-frame label map (the way in of the labels; the frames' way in is csrc/frame_resize.hip).
// The reference's YouTube-VOS fork ends track() with interpolate(y, sz) (bilinear, align_corners=False, the identity on equal sizes):
// that is the operator here, bilinear_taps of resample_taps.h being its definition.
//
//   m_k    = the bilinear sample of plane k at the native pixel (the plane itself when the sizes agree),
//   arg    = the first k with the largest m_k,
//   label  = lut[arg] if arg >= 1 and m_arg > 0.5, else lut[0]
//
// which is what k_track_merge's two decode branches (target_model.hip) reduce to on MERGED masks, where every plane but the winner is 0:
// on equal sizes the labels are byte for byte frtm_track_merge's.
#include "frtm_common.h"
#include "resample_taps.h"
#include "per_frame.h"       // MERGE_MAX: the planes of one merged frame
#include "../../include/frtm_hip.h"
#include <cstdint>

#define NS_TH 16            // output tile: rows (thread (tx, tg) owns rows tg + 4 i)
#define NS_TW 64            //              columns: lane = column, so a wave writes 64 consecutive label bytes / 256 consecutive mask bytes
#define NS_PR 36            // source rows per staged chunk: a tile that enlarges, or reduces by up to 2, is ONE chunk (16 * 2 + 2 rows)
#define NS_PC 132           // source columns per staged chunk (64 * 2 + 2), + 1 word of padding per LDS row
#define NS_PCP (NS_PC + 1)
#define NS_MAXDIM 16384     // FR_MAXDIM of frame_resize.hip
#define NS_ROW 7            // 64-bit words per table row

// Does row r name a frame inside the buffers?  (Evaluated by the kernel from the DEVICE table and by the host, for the grid, from its copy.)
__host__ __device__ static inline bool ns_row_ok(const long long* r, int h, int w, long long mask_elems, long long label_bytes, long long soft_elems,
                                                  long long lut_bytes) {
  const long long moff = r[0], K = r[1], H = r[2], W = r[3], loff = r[4], soff = r[5], toff = r[6];
  if (K < 1 || K > MERGE_MAX || H < 1 || W < 1 || H > NS_MAXDIM || W > NS_MAXDIM) return false;
  if (moff < 0 || moff > mask_elems || K * h * w > mask_elems - moff) return false;
  if (loff < 0 || loff > label_bytes || H * W > label_bytes - loff) return false;
  if (soff != -1 && (soff < 0 || soff > soft_elems || K * H * W > soft_elems - soff)) return false;
  if (toff < 0 || toff > lut_bytes || K > lut_bytes - toff) return false;
  return true;
}

// One workgroup = one NS_TH x NS_TW native tile of one frame, all its planes one after the other.  Per plane the tile's source footprint
// (rows R0 .. R1, columns C0 .. C1 of the working-size plane) is staged in LDS in chunks of NS_PR x NS_PC -- one chunk unless the native
// frame is less than half the working size -- and every thread picks the four taps of each of its four outputs out of the chunk that
// holds them; the sample is then bilinear_at's expression on those four values, so a source row is read from memory once per tile.
__global__ __launch_bounds__(256) void k_masks_to_native(const float* __restrict__ masks, long long mask_elems, int h, int w,
                                                          const long long* __restrict__ table, unsigned char* __restrict__ labels,
                                                          long long label_bytes, float* __restrict__ soft, long long soft_elems,
                                                          const unsigned char* __restrict__ luts, long long lut_bytes) {
  __shared__ float patch[NS_PR * NS_PCP];
  const long long* row = table + (size_t)NS_ROW * blockIdx.z;
  if (!ns_row_ok(row, h, w, mask_elems, label_bytes, soft ? soft_elems : 0, lut_bytes)) return;      // (uniform per workgroup, before any barrier)
  const int K = (int)row[1], H = (int)row[2], W = (int)row[3];
  const int y0 = blockIdx.y * NS_TH, x0 = blockIdx.x * NS_TW;
  if (y0 >= H || x0 >= W) return;                                       // (the grid is sized for the launch's largest frame)
  const float* msrc = masks + row[0];
  unsigned char* lab = labels + row[4];
  float* sdst = row[5] >= 0 ? soft + row[5] : nullptr;
  const unsigned char* lut = luts + row[6];
  const bool same = h == H && w == W;
  const float sy = (float)h / (float)H, sx = (float)w / (float)W;      // bilinear_at's scales
  const int th = min(NS_TH, H - y0), tw = min(NS_TW, W - x0);
  const int tx = threadIdx.x & 63, tg = threadIdx.x >> 6;
  const bool col_ok = tx < tw;
  const int xo = x0 + min(tx, tw - 1);

  int xa, xb; float lx0, lx1;                                          // this lane's column taps
  bilinear_taps(xo, sx, w, xa, xb, lx0, lx1);
  int ya[4], yb[4]; float ly0[4], ly1[4];                              // row taps of the outputs (tg + 4 i, tx)
#pragma unroll
  for (int i = 0; i < 4; ++i) bilinear_taps(y0 + min(tg + 4 * i, th - 1), sy, h, ya[i], yb[i], ly0[i], ly1[i]);
  if (same) { xa = xb = xo; }
  int R0, R1, C0, C1, t0, t1; float f0, f1;                            // the tile's footprint (taps are monotonic in the output index)
  bilinear_taps(y0, sy, h, R0, t1, f0, f1);
  bilinear_taps(y0 + th - 1, sy, h, t0, R1, f0, f1);
  bilinear_taps(x0, sx, w, C0, t1, f0, f1);
  bilinear_taps(x0 + tw - 1, sx, w, t0, C1, f0, f1);

  float best[4]; int arg[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { best[i] = -INFINITY; arg[i] = 0; }

  for (int k = 0; k < K; ++k) {
    const float* pl = msrc + (size_t)k * h * w;
    float v00[4], v01[4], v10[4], v11[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v00[i] = v01[i] = v10[i] = v11[i] = 0.f;
    for (int rc0 = R0; rc0 <= R1; rc0 += NS_PR) {
      const int rcn = min(NS_PR, R1 - rc0 + 1);
      for (int cc0 = C0; cc0 <= C1; cc0 += NS_PC) {
        const int ccn = min(NS_PC, C1 - cc0 + 1);
        __syncthreads();                                               // the previous chunk's readers are done with the patch
        for (int r = tg; r < rcn; r += 4) {                            // a wave per source row: consecutive lanes, consecutive words
          const float* srow = pl + (size_t)(rc0 + r) * w + cc0;
          for (int c = tx; c < ccn; c += 64) patch[r * NS_PCP + c] = srow[c];
        }
        __syncthreads();
        const bool ina = xa >= cc0 && xa < cc0 + ccn, inb = xb >= cc0 && xb < cc0 + ccn;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (ya[i] >= rc0 && ya[i] < rc0 + rcn) {
            const float* p = patch + (ya[i] - rc0) * NS_PCP - cc0;
            if (ina) v00[i] = p[xa];
            if (inb) v01[i] = p[xb];
          }
          if (yb[i] >= rc0 && yb[i] < rc0 + rcn) {
            const float* p = patch + (yb[i] - rc0) * NS_PCP - cc0;
            if (ina) v10[i] = p[xa];
            if (inb) v11[i] = p[xb];
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // bilinear_at: the map itself when the sizes agree, else its expression
      const float m = same ? v00[i] : ly0[i] * (lx0 * v00[i] + lx1 * v01[i]) + ly1[i] * (lx0 * v10[i] + lx1 * v11[i]);
      merged_offer(m, k, best[i], arg[i]);
      if (sdst && col_ok && tg + 4 * i < th) sdst[((size_t)k * H + (y0 + tg + 4 * i)) * W + xo] = m;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (col_ok && tg + 4 * i < th) lab[(size_t)(y0 + tg + 4 * i) * W + xo] = lut[merged_plane(arg[i], best[i])];
}

// k_resize_labels of frame_resize.hip with the id copied instead of compared: the same source index, the same float32 product.
__global__ __launch_bounds__(256) void k_resize_label_map(const unsigned char* __restrict__ src, const long long* __restrict__ desc,
                                                           unsigned char* __restrict__ out, int H, int W) {
  const int f = blockIdx.y;
  const int h = (int)desc[4 * f + 1], w = (int)desc[4 * f + 2];
  const unsigned char* s = src + desc[4 * f];
  const float sy = __fdiv_rn((float)h, (float)H), sx = __fdiv_rn((float)w, (float)W);
  const int total = H * W;
  for (int pix = blockIdx.x * 256 + threadIdx.x; pix < total; pix += gridDim.x * 256) {
    const int y = pix / W, x = pix - y * W;
    const int ys = min((int)floorf(__fmul_rn((float)y, sy)), h - 1), xs = min((int)floorf(__fmul_rn((float)x, sx)), w - 1);
    out[(size_t)f * total + pix] = s[(size_t)ys * w + xs];
  }
}

extern "C" int frtm_masks_to_native(const float* masks, size_t mask_elems, int h, int w, const long long* table_host, const long long* table_dev,
                                    int n, unsigned char* labels, size_t label_bytes, float* soft, size_t soft_elems, const unsigned char* luts,
                                    size_t lut_bytes, frtm_stream_t stream) {
  FRTM_CHECK_ARG(masks && table_host && table_dev && labels && luts && n >= 1 && n <= 65535, "frtm_masks_to_native: bad argument");
  FRTM_CHECK_ARG(h >= 1 && w >= 1 && h <= NS_MAXDIM && w <= NS_MAXDIM, "frtm_masks_to_native: working size %d x %d (1 .. %d)", h, w, NS_MAXDIM);
  FRTM_CHECK_ARG(mask_elems < ((size_t)1 << 62) && label_bytes < ((size_t)1 << 62) && soft_elems < ((size_t)1 << 62) && lut_bytes < ((size_t)1 << 62),
                 "frtm_masks_to_native: a buffer size is not a size");
  int maxH = 0, maxW = 0;
  for (int i = 0; i < n; ++i) {
    const long long* r = table_host + (size_t)NS_ROW * i;
    FRTM_CHECK_ARG(r[1] >= 1 && r[1] <= MERGE_MAX, "frtm_masks_to_native: frame %d has %lld planes (1 .. %d)", i, r[1], MERGE_MAX);
    FRTM_CHECK_ARG(r[2] >= 1 && r[3] >= 1 && r[2] <= NS_MAXDIM && r[3] <= NS_MAXDIM, "frtm_masks_to_native: frame %d has native size %lld x %lld (1 .. %d)",
                   i, r[2], r[3], NS_MAXDIM);
    FRTM_CHECK_ARG(r[5] == -1 || soft, "frtm_masks_to_native: frame %d asks for soft planes, but there is no soft buffer", i);
    // a row whose frame leaves a buffer is not an error: the kernel skips it and writes nothing (ragged_group.hip's rule)
    if (!ns_row_ok(r, h, w, (long long)mask_elems, (long long)label_bytes, soft ? (long long)soft_elems : 0, (long long)lut_bytes)) continue;
    maxH = max(maxH, (int)r[2]);
    maxW = max(maxW, (int)r[3]);
  }
  if (maxH == 0) return FRTM_OK;                                       // no row names a frame
  dim3 g(ceil_div(maxW, NS_TW), ceil_div(maxH, NS_TH), n);
  k_masks_to_native<<<g, 256, 0, (hipStream_t)stream>>>(masks, (long long)mask_elems, h, w, table_dev, labels, (long long)label_bytes, soft,
                                                         soft ? (long long)soft_elems : 0, luts, (long long)lut_bytes);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

extern "C" int frtm_resize_label_map_u8(const unsigned char* src, size_t src_bytes, const long long* desc_host, const long long* desc_dev, int n,
                                        unsigned char* out, int H, int W, frtm_stream_t stream) {
  FRTM_CHECK_ARG(src && desc_host && desc_dev && out && n >= 1 && n <= 65535, "frtm_resize_label_map_u8: bad argument");
  FRTM_CHECK_ARG(H >= 1 && W >= 1 && H <= NS_MAXDIM && W <= NS_MAXDIM, "frtm_resize_label_map_u8: output size %d x %d (1 .. %d)", H, W, NS_MAXDIM);
  for (int i = 0; i < n; ++i) {                                        // rows {byte offset, h, w, 0}: the frame's bytes must lie inside [0, src_bytes)
    const long long off = desc_host[4 * i], h = desc_host[4 * i + 1], w = desc_host[4 * i + 2];
    FRTM_CHECK_ARG(h >= 1 && w >= 1 && h <= NS_MAXDIM && w <= NS_MAXDIM, "frtm_resize_label_map_u8: frame %d has size %lld x %lld (1 .. %d)", i, h, w, NS_MAXDIM);
    FRTM_CHECK_ARG(desc_host[4 * i + 3] == 0, "frtm_resize_label_map_u8: frame %d: the fourth word of a row is 0", i);
    FRTM_CHECK_ARG(off >= 0 && (size_t)off <= src_bytes && (size_t)h * (size_t)w <= src_bytes - (size_t)off,
                   "frtm_resize_label_map_u8: frame %d (offset %lld, %lld x %lld bytes) leaves the %zu-byte source buffer", i, off, h, w, src_bytes);
  }
  dim3 g((unsigned)min(ceil_div(H * W, 256), 1024), n);
  k_resize_label_map<<<g, 256, 0, (hipStream_t)stream>>>(src, desc_dev, out, H, W);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}
