// The resize operator of csrc/frame_resize.hip, stated ONCE for the kernels that run it: k_resize_frames (frame_resize.hip: packed planar
// frames) and k_frames_to_rgb (frame_formats.hip: decoder surfaces, colour conversion fused in front).  What differs between them is how a
// chunk of the source footprint gets into LDS (the Stage argument of resize_tile); the tap positions, the weights, the summation order of
// the two passes and the one rounding at the end are these lines for both, so their results agree bit for bit by construction.
#ifndef FRTM_FRAME_PASSES_H_
#define FRTM_FRAME_PASSES_H_
#include <hip/hip_runtime.h>
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

// Rows rc0 .. rc0 + rcn - 1, columns cc0 .. cc0 + ccn - 1 of one h x w byte plane that lies inside the frame [fsrc, fend) into ``patch``:
// 16-byte loads from 16-byte aligned ADDRESSES -- a row of a packed frame starts anywhere, so each LDS row keeps its own phase
// (address & 15, plane_phase) and the words that straddle the frame's first or last byte are read byte by byte.
__device__ __forceinline__ void stage_plane(unsigned char* patch, const unsigned char* psrc, const unsigned char* fsrc, const unsigned char* fend,
                                            int w, int rc0, int rcn, int cc0, int ccn) {
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
}

__device__ __forceinline__ int plane_phase(const unsigned char* psrc, int w, int row, int cc0) {
  return (int)((uintptr_t)(psrc + (size_t)row * w + cc0) & 15);
}

// One workgroup (256 threads) = the FR_TH x FR_TW output tile (blockIdx.y, blockIdx.x) of one H x W output plane ``oplane`` whose source
// is an h x w byte plane.  The tile's source footprint is walked in chunks of FR_PR rows x FR_PC columns (a 1.5x reduction fits one chunk;
// a larger ratio loops): ``stage.fill(patch, rc0, rcn, cc0, ccn)`` puts the chunk's bytes into LDS, row r of the chunk at
// patch + r * FR_PCB + stage.phase(rc0 + r, cc0); then the horizontal pass leaves one fp32 value per (chunk row, output column) and the
// vertical pass adds the chunk's share to the four outputs a thread owns.  patch: FR_PR * FR_PCB bytes of LDS, 16-byte aligned; hrow:
// FR_PR * FR_TW floats of LDS.
template <class Stage>
__device__ __forceinline__ void resize_tile(const Stage& stage, int mode, int h, int w, unsigned char* __restrict__ oplane, int H, int W,
                                            unsigned char* patch, float* hrow) {
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
      stage.fill(patch, rc0, rcn, cc0, ccn);
      __syncthreads();
      int lb[FR_PR / 4];                                               // LDS offset of source column 0 in this thread's rows
#pragma unroll
      for (int i = 0; i < FR_PR / 4; ++i) {
        const int r = tg + 4 * i;
        lb[i] = r * FR_PCB + stage.phase(rc0 + r, cc0) - cc0;
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
    if (col_ok && tg + 4 * i < th) oplane[(size_t)y * W + xo] = (unsigned char)fminf(fmaxf(rintf(acc[i]), 0.f), 255.f);
  }
}

#endif  // FRTM_FRAME_PASSES_H_
