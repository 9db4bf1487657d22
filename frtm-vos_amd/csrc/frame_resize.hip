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
#include "frame_passes.h"

// Axis, axis_span, axis_weight and the two passes: frame_passes.h, shared with csrc/frame_formats.hip.

// The Stage of resize_tile for a plane of a packed planar frame.
struct PackedPlane {
  const unsigned char *psrc, *fsrc, *fend;                             // the plane; the frame [fsrc, fend) it lies in
  int w;
  __device__ __forceinline__ void fill(unsigned char* patch, int rc0, int rcn, int cc0, int ccn) const {
    stage_plane(patch, psrc, fsrc, fend, w, rc0, rcn, cc0, ccn);
  }
  __device__ __forceinline__ int phase(int row, int cc0) const { return plane_phase(psrc, w, row, cc0); }
};

// One workgroup = one FR_TH x FR_TW output tile of one plane of one frame (resize_tile).
__global__ __launch_bounds__(256) void k_resize_frames(const unsigned char* __restrict__ src, const long long* __restrict__ desc, int planes,
                                                        unsigned char* __restrict__ out, int H, int W) {
  __shared__ __attribute__((aligned(16))) unsigned char patch[FR_PR * FR_PCB];
  __shared__ float hrow[FR_PR * FR_TW];
  const int f = blockIdx.z / planes, pl = blockIdx.z - f * planes;
  const int h = (int)desc[4 * f + 1], w = (int)desc[4 * f + 2], mode = (int)desc[4 * f + 3];
  PackedPlane st;
  st.fsrc = src + desc[4 * f];                                         // the frame: planes * h * w bytes
  st.fend = st.fsrc + (size_t)planes * h * w;
  st.psrc = st.fsrc + (size_t)pl * h * w;
  st.w = w;
  resize_tile(st, mode, h, w, out + (size_t)blockIdx.z * H * W, H, W, patch, hrow);
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
