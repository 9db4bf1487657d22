// Decoder frames in, planar RGB at the step size out: a hardware video decoder leaves an NV12 surface on the device -- a Y plane of
// pitch-wide rows, then one plane of interleaved U,V at half resolution, the pitch larger than the width and the coded height larger than
// the picture -- and the tracker reads (3, H, W) uint8 planes.  k_frames_to_rgb converts and resizes in one launch: each workgroup stages
// the CONVERTED bytes of its source footprint in LDS and then runs the passes of k_resize_frames on them (frame_passes.h: the same lines),
// so the result is, bit for bit, the resize of the converted planes.  Planar RGB rows (format 0) take k_resize_frames' own staging.
//
// The conversion is one fixed-point formula (include/frtm_hip.h), chroma replicated over its 2 x 2 block:
//   Y = buf[off + y pitch + x], U = buf[uv_off + (y >> 1) pitch + 2 (x >> 1)], V = the byte after U
//   yy = Y - y0, u = U - 128, v = V - 128;  R = clamp((a yy + rv v + 32768) >> 16), G = clamp((a yy - gu u - gv v + 32768) >> 16),
//   B = clamp((a yy + bu u + 32768) >> 16), the shift arithmetic (floor), the clamp to 0..255; every intermediate is below 6e7.
// Loads: bytes at the addresses above only, for x < w and y < h -- never a byte of the row padding, of the rows between the picture and
// the coded height or of a neighbouring frame, so the result cannot depend on one.
#include "frtm_common.h"
#include "frame_passes.h"

// {y0, a, rv, gu, gv, bu} of formats 1 .. 4: round(65536 * coefficient) of BT.601 / BT.709, limited / full range
__constant__ int kYuv[4][6] = {
    {16, 76309, 104597, 25675, 53279, 132201},
    {0, 65536, 91881, 22553, 46802, 116130},
    {16, 76309, 117489, 13975, 34925, 138438},
    {0, 65536, 103206, 12276, 30679, 121609},
};

// The Stage of resize_tile for plane ``pl`` (0 R, 1 G, 2 B) of one frame of any format.
struct FramePlane {
  int format, w;
  // format 0
  const unsigned char *psrc, *fsrc, *fend;
  // NV12: the two planes, their pitch, and this colour plane's row of the matrix: value = (a yy + cu u + cv v + 32768) >> 16
  const unsigned char *ysrc, *uvsrc;
  long long pitch;
  int y0, a, cu, cv;

  __device__ __forceinline__ void fill(unsigned char* patch, int rc0, int rcn, int cc0, int ccn) const {
    if (format == FRTM_FRAME_RGB) {
      stage_plane(patch, psrc, fsrc, fend, w, rc0, rcn, cc0, ccn);
      return;
    }
    // one thread per chroma pair of a row: columns 2 p and 2 p + 1; a chunk that starts or ends in the middle of a pair takes its half of it
    const int p0 = cc0 >> 1, np = ((cc0 + ccn - 1) >> 1) - p0 + 1;
    for (int it = threadIdx.x; it < rcn * np; it += 256) {
      const int r = it / np, p = p0 + (it - r * np);
      const int y = rc0 + r;                                           // < h: the chunk lies inside the picture
      const unsigned char* uv = uvsrc + (size_t)(y >> 1) * pitch + 2 * p;
      const int c = cu * ((int)uv[0] - 128) + cv * ((int)uv[1] - 128) + 32768;
      const unsigned char* yrow = ysrc + (size_t)y * pitch;
      unsigned char* lds = patch + r * FR_PCB - cc0;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int x = 2 * p + k;
        if (x < cc0 || x >= cc0 + ccn) continue;                       // (cc0 + ccn <= w)
        lds[x] = (unsigned char)min(max((a * ((int)yrow[x] - y0) + c) >> 16, 0), 255);
      }
    }
  }
  __device__ __forceinline__ int phase(int row, int cc0) const { return format == FRTM_FRAME_RGB ? plane_phase(psrc, w, row, cc0) : 0; }
};

// One workgroup = one FR_TH x FR_TW output tile of one colour plane of one frame; blockIdx.z = 3 * frame + plane.
__global__ __launch_bounds__(256) void k_frames_to_rgb(const unsigned char* __restrict__ src, const long long* __restrict__ desc,
                                                        unsigned char* __restrict__ out, int H, int W) {
  __shared__ __attribute__((aligned(16))) unsigned char patch[FR_PR * FR_PCB];
  __shared__ float hrow[FR_PR * FR_TW];
  const int f = blockIdx.z / 3, pl = blockIdx.z - 3 * f;
  const long long* d = desc + 8 * f;
  const int h = (int)d[1], w = (int)d[2], mode = (int)d[3];
  FramePlane st;
  st.format = (int)d[4];
  st.w = w;
  st.fsrc = st.ysrc = src + d[0];
  st.fend = st.fsrc + (size_t)3 * h * w;
  st.psrc = st.fsrc + (size_t)pl * h * w;
  st.pitch = d[5];
  st.uvsrc = src + d[6];
  st.y0 = st.a = st.cu = st.cv = 0;
  if (st.format != FRTM_FRAME_RGB) {
    const int* k = kYuv[st.format - 1];
    st.y0 = k[0];
    st.a = k[1];
    st.cu = pl == 0 ? 0 : pl == 1 ? -k[3] : k[5];
    st.cv = pl == 0 ? k[2] : pl == 1 ? -k[4] : 0;
  }
  resize_tile(st, mode, h, w, out + (size_t)blockIdx.z * H * W, H, W, patch, hrow);
}

extern "C" int frtm_frames_to_rgb_u8(const unsigned char* src, size_t src_bytes, const long long* desc_host, const long long* desc_dev, int n,
                                     unsigned char* out, int H, int W, frtm_stream_t stream) {
  const char* who = "frtm_frames_to_rgb_u8";
  FRTM_CHECK_ARG(src && desc_host && desc_dev && out && n >= 1, "%s: bad argument (a null pointer or n < 1)", who);
  FRTM_CHECK_ARG(H >= 1 && W >= 1 && H <= FR_MAXDIM && W <= FR_MAXDIM, "%s: output size %d x %d (1 .. %d)", who, H, W, FR_MAXDIM);
  FRTM_CHECK_ARG(3LL * n <= 65535, "%s: at most 65535 planes per call (%d frames)", who, n);
  for (int i = 0; i < n; ++i) {
    const long long* d = desc_host + 8 * i;
    const long long off = d[0], h = d[1], w = d[2], mode = d[3], format = d[4], pitch = d[5], uv_off = d[6];
    FRTM_CHECK_ARG(h >= 1 && w >= 1 && h <= FR_MAXDIM && w <= FR_MAXDIM, "%s: frame %d has size %lld x %lld (1 .. %d)", who, i, h, w, FR_MAXDIM);
    FRTM_CHECK_ARG(mode == FRTM_RESIZE_AREA || mode == FRTM_RESIZE_CUBIC, "%s: frame %d has mode %lld (%d .. %d)", who, i, mode, FRTM_RESIZE_AREA,
                   FRTM_RESIZE_CUBIC);
    FRTM_CHECK_ARG(format >= FRTM_FRAME_RGB && format <= FRTM_FRAME_NV12_BT709_FULL, "%s: frame %d has format %lld (%d .. %d)", who, i, format,
                   FRTM_FRAME_RGB, FRTM_FRAME_NV12_BT709_FULL);
    if (format == FRTM_FRAME_RGB) {
      FRTM_CHECK_ARG(off >= 0 && (size_t)off <= src_bytes && 3 * (size_t)h * (size_t)w <= src_bytes - (size_t)off,
                     "%s: frame %d (offset %lld, 3 x %lld x %lld bytes) leaves the %zu-byte source buffer", who, i, off, h, w, src_bytes);
      continue;
    }
    FRTM_CHECK_ARG(pitch >= 2 * ((w + 1) / 2), "%s: frame %d has pitch %lld, below its %lld-byte chroma row", who, i, pitch, 2 * ((w + 1) / 2));
    // (pitch <= src_bytes first: the products below then stay far from 2^63)
    const bool y_in = off >= 0 && (size_t)off <= src_bytes && (size_t)pitch <= src_bytes && (size_t)pitch * (size_t)h <= src_bytes - (size_t)off;
    FRTM_CHECK_ARG(y_in, "%s: frame %d's Y plane (offset %lld, %lld rows of pitch %lld) leaves the %zu-byte source buffer", who, i, off, h, pitch,
                   src_bytes);
    const bool uv_in = uv_off >= 0 && (size_t)uv_off <= src_bytes && (size_t)pitch * (size_t)((h + 1) / 2) <= src_bytes - (size_t)uv_off;
    FRTM_CHECK_ARG(uv_in, "%s: frame %d's chroma plane (offset %lld, %lld rows of pitch %lld) leaves the %zu-byte source buffer", who, i, uv_off,
                   (h + 1) / 2, pitch, src_bytes);
  }
  dim3 g(ceil_div(W, FR_TW), ceil_div(H, FR_TH), 3 * n);
  k_frames_to_rgb<<<g, 256, 0, (hipStream_t)stream>>>(src, desc_dev, out, H, W);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}
