// Grouped target-model scoring for gfx950: G (frame, target) pairs in one call -- what G calls of Discriminator.apply_window on one
// frame each compute, without their 3 G small launches (split-K 1x1 projection, its epilogue, 3x3 filter).
//
//   k_grouped_project   cft[p] = w1T[p]^T X[frame_of_pair[p]]      fp32 MFMA (v_mfma_f32_16x16x4_f32), grid (column tiles, 1, G)
//   k_grouped_scores    scores[p] = w2[p] * cft[p]  (3x3, zero padding)  grid (pixel tiles, G)
//
// No split-K and no atomics: every output element of the projection is ONE chain over K = Cin in ascending order (the MFMA's own
// k order inside a step, the steps and the 32-deep chunks in order), whatever the tile and whatever else is in the launch; the
// parallelism that split-K buys a single pair comes from the pairs.  The 3x3 pass has one fixed summation order.  Workgroups of
// different pairs share nothing, so a pair's result does not depend on G, on its place in the tables or on the other pairs.
#include "frtm_common.h"
#include "../../include/frtm_hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int GP_BK = 32;       // K chunk: Cin must be a multiple of it
constexpr int GP_NT = 256;      // 4 waves = 2 (rows) x 2 (columns)

// Tile = (2 * FM * 16 rows: all c <= 128 projected channels) x (2 * FN * 16 pixels).  A = w1T chunk [k][m] and B = feature chunk [k][n],
// both in their natural layouts, staged through registers into double-buffered LDS: one barrier per chunk.
template <int FM, int FN>
__global__ __launch_bounds__(GP_NT) void k_grouped_project(const float* __restrict__ feats, size_t frame_pitch, int F,
                                                            const int* __restrict__ frame_of_pair, const float* const* __restrict__ w1T_tab,
                                                            int Cin, int c, int hw, float* __restrict__ cft) {
  constexpr int BM = 2 * FM * 16, BN = 2 * FN * 16;
  constexpr int LDA = BM + 16, LDB = BN + 16;          // row pitch = 16 mod 32 banks apart for the 4 k rows a fragment read touches
  constexpr int EA = GP_BK * BM / GP_NT, EB = GP_BK * BN / GP_NT;
  __shared__ float As[2][GP_BK][LDA];
  __shared__ float Bs[2][GP_BK][LDB];
  const int p = blockIdx.z;
  const int frame = frame_of_pair[p];
  if ((unsigned)frame >= (unsigned)F) return;          // (uniform per workgroup) a pair that names no frame of the batch writes nothing
  const float* __restrict__ A = w1T_tab[p];
  const float* __restrict__ X = feats + (size_t)frame * frame_pitch;
  const int n0 = blockIdx.x * BN;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int wm = wid >> 1, wn = wid & 1;

  // what this thread stages per chunk: EA elements of the (32 x c, contiguous) block of w1T, EB of the 32 x BN feature block
  int a_src[EA], a_dst[EA];
#pragma unroll
  for (int e = 0; e < EA; ++e) {
    const int idx = tid + e * GP_NT;
    const bool ok = idx < GP_BK * c;
    const int k = ok ? idx / c : 0, m = ok ? idx - k * c : 0;
    a_src[e] = ok ? idx : -1;
    a_dst[e] = k * LDA + m;
  }
  int b_src[EB], b_dst[EB];
#pragma unroll
  for (int e = 0; e < EB; ++e) {
    const int idx = tid + e * GP_NT;
    const int k = idx / BN, n = idx - k * BN;
    b_src[e] = (n0 + n < hw) ? k * hw + n0 + n : -1;
    b_dst[e] = k * LDB + n;
  }
  // rows c..BM-1 of A and the columns past the map are never staged: zero both buffers once
  for (int i = tid; i < 2 * GP_BK * LDA; i += GP_NT) (&As[0][0][0])[i] = 0.f;
  for (int i = tid; i < 2 * GP_BK * LDB; i += GP_NT) (&Bs[0][0][0])[i] = 0.f;
  __syncthreads();

  float ra[EA], rb[EB];
  auto gload = [&](int kc) {
    const float* Ac = A + (size_t)kc * GP_BK * c;
    const float* Xc = X + (size_t)kc * GP_BK * hw;
#pragma unroll
    for (int e = 0; e < EA; ++e) ra[e] = a_src[e] >= 0 ? Ac[a_src[e]] : 0.f;
#pragma unroll
    for (int e = 0; e < EB; ++e) rb[e] = b_src[e] >= 0 ? Xc[b_src[e]] : 0.f;
  };
  auto lstore = [&](int buf) {
    float* as = &As[buf][0][0];
    float* bs = &Bs[buf][0][0];
#pragma unroll
    for (int e = 0; e < EA; ++e)
      if (a_src[e] >= 0) as[a_dst[e]] = ra[e];
#pragma unroll
    for (int e = 0; e < EB; ++e) bs[b_dst[e]] = rb[e];
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = Cin / GP_BK;
  gload(0);
  lstore(0);
  __syncthreads();
  for (int kc = 0; kc < nchunks; ++kc) {
    const int cur = kc & 1;
    const bool more = kc + 1 < nchunks;
    if (more) gload(kc + 1);
#pragma unroll
    for (int kk = 0; kk < GP_BK / 4; ++kk) {
      float af[FM], bf[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) af[i] = As[cur][kk * 4 + lk][(wm * FM + i) * 16 + li];
#pragma unroll
      for (int j = 0; j < FN; ++j) bf[j] = Bs[cur][kk * 4 + lk][(wn * FN + j) * 16 + li];
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    if (more) lstore(cur ^ 1);      // (the other buffer: its readers passed the barrier that ended chunk kc - 1)
    __syncthreads();
  }

  // C/D layout of the 16x16 MFMA: column = lane & 15, row = (lane >> 4) * 4 + reg
  float* out = cft + (size_t)p * c * hw;
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + (wn * FN + j) * 16 + li;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = (wm * FM + i) * 16 + lk * 4 + r;
        if (m < c && n < hw) out[(size_t)m * hw + n] = acc[i][j][r];
      }
    }
}

// frtm_filter_scores' pixel form (16 pixels per workgroup, 16 channel groups) with the pair's features and filter taken from the
// tables: each lane walks its channels in ascending order, 9 taps each; the 4 channel groups of a wave are added by a butterfly
// and the 4 waves as (0 + 1) + (2 + 3).  One form for every G: a pair's scores do not depend on the launch they are part of.
constexpr int GS_PX = 16;
__global__ __launch_bounds__(256) void k_grouped_scores(const float* __restrict__ cft, int F, const int* __restrict__ frame_of_pair,
                                                         const float* const* __restrict__ w2_tab, int C, int h, int w,
                                                         float* __restrict__ scores) {
  constexpr int CGW = 64 / GS_PX, NG = 4 * CGW;
  __shared__ float red[4][GS_PX];
  const int pair = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // (uniform per workgroup, before the barrier) the projection wrote no features for a pair that names no frame of the batch: cft[pair]
  // holds whatever the workspace held, so neither read it nor write scores[pair]
  if ((unsigned)frame_of_pair[pair] >= (unsigned)F) return;
  const int pl = lane % GS_PX, cg = wid * CGW + lane / GS_PX;
  const int hw = h * w;
  const int px_ = blockIdx.x * GS_PX + pl;
  const bool live = px_ < hw;
  const int py = live ? px_ / w : 0, px = live ? px_ % w : 0;
  bool ok[9]; int off[9];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int yy = py + dy - 1, xx = px + dx - 1;
      const bool v = live && (unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w;
      ok[dy * 3 + dx] = v;
      off[dy * 3 + dx] = v ? yy * w + xx : 0;
    }
  const int cper = (C + NG - 1) / NG;
  const int c0 = cg * cper, c1 = min(C, c0 + cper);
  const float* __restrict__ Xn = cft + (size_t)pair * C * hw;
  const float* __restrict__ f = w2_tab[pair];
  float acc = 0.f;
  for (int ch = c0; ch < c1; ++ch) {
    const float* Xc = Xn + (size_t)ch * hw;
    const float* fc = f + ch * 9;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const float v = Xc[off[k]];
      acc += (ok[k] ? v : 0.f) * fc[k];
    }
  }
#pragma unroll
  for (int o = GS_PX; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);
  if (lane < GS_PX) red[wid][lane] = acc;
  __syncthreads();
  if (wid == 0 && lane < GS_PX && live)
    scores[(size_t)pair * hw + px_] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

template <int FM>
static void launch_project(int FN, dim3 grid, hipStream_t st, const float* feats, size_t pitch, int F, const int* fop, const float* const* w1T,
                           int Cin, int c, int hw, float* cft) {
  if (FN == 1) k_grouped_project<FM, 1><<<grid, GP_NT, 0, st>>>(feats, pitch, F, fop, w1T, Cin, c, hw, cft);
  else k_grouped_project<FM, 2><<<grid, GP_NT, 0, st>>>(feats, pitch, F, fop, w1T, Cin, c, hw, cft);
}

// The one definition of the projection's tile: FM = 16-row MFMA blocks per wave row (2 * FM * 16 >= c rows), FN = 1 or 2 column blocks per
// wave column.  64-column tiles (FN = 2) read each pair's features once and fill the 256 CUs from G = 10 at 30x54; below a chip's worth of
// those, 32-column tiles (twice the workgroups).  Same chain per output element either way.
int frtm_target_apply_grouped_tiles(int G, int c, int h, int w, int* fm, int* fn) {
  FRTM_CHECK_ARG(G >= 1 && G <= 65535 && h >= 1 && w >= 1 && (long long)h * w <= (1 << 24) && c >= 1 && c <= 128 && fm && fn,
                 "frtm_target_apply_grouped_tiles: needs 1 <= G <= 65535, 1 <= c <= 128, a non-empty map of at most 2^24 pixels (got G=%d c=%d %dx%d)",
                 G, c, h, w);
  *fm = ceil_div(c, 32);
  *fn = ((long long)ceil_div(h * w, 64) * G >= 256) ? 2 : 1;
  return FRTM_OK;
}

int frtm_target_apply_grouped(const float* feats, size_t frame_pitch, int F, const int* frame_of_pair, const float* const* w1T,
                              const float* const* w2, int G, int Cin, int c, int h, int w, float* cft, float* scores, frtm_stream_t stream) {
  FRTM_CHECK_ARG(feats && frame_of_pair && w1T && w2 && cft && scores, "frtm_target_apply_grouped: null argument");
  FRTM_CHECK_ARG(G >= 1 && G <= 65535 && F >= 1 && h >= 1 && w >= 1, "frtm_target_apply_grouped: needs 1 <= G <= 65535 pairs, F >= 1 frames and a non-empty map (got G=%d F=%d %dx%d)", G, F, h, w);
  FRTM_CHECK_ARG(c >= 1 && c <= 128, "frtm_target_apply_grouped: at most 128 projected channels (got c=%d)", c);
  FRTM_CHECK_ARG(Cin >= GP_BK && Cin % GP_BK == 0, "frtm_target_apply_grouped: Cin must be a multiple of %d (got %d)", GP_BK, Cin);
  FRTM_CHECK_ARG((long long)h * w <= (1 << 24) && (long long)Cin * h * w <= 0x7fffffffLL && frame_pitch >= (size_t)Cin * h * w,
                 "frtm_target_apply_grouped: map %dx%d x %d channels too large, or frame pitch %zu below Cin*h*w", h, w, Cin, frame_pitch);
  hipStream_t st = (hipStream_t)stream;
  const int hw = h * w;
  int FM, FN;
  if (frtm_target_apply_grouped_tiles(G, c, h, w, &FM, &FN) != FRTM_OK) return FRTM_ERR_ARG;
  dim3 grid(ceil_div(hw, FN * 32), 1, G);
  switch (FM) {
    case 1: launch_project<1>(FN, grid, st, feats, frame_pitch, F, frame_of_pair, w1T, Cin, c, hw, cft); break;
    case 2: launch_project<2>(FN, grid, st, feats, frame_pitch, F, frame_of_pair, w1T, Cin, c, hw, cft); break;
    case 3: launch_project<3>(FN, grid, st, feats, frame_pitch, F, frame_of_pair, w1T, Cin, c, hw, cft); break;
    default: launch_project<4>(FN, grid, st, feats, frame_pitch, F, frame_of_pair, w1T, Cin, c, hw, cft); break;
  }
  FRTM_LAUNCH_CHECK();
  dim3 g2(ceil_div(hw, GS_PX), G);
  k_grouped_scores<<<g2, 256, 0, st>>>(cft, F, frame_of_pair, w2, c, h, w, scores);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}
