// What a program that ACTS on the answer needs, measured on the device: per object of a frame its area, box, coordinate sums, edge and border
// pixels, confidence and soft area -- for all frames of a tick, label maps and merged mask stacks of any sizes, in ONE launch
// (ops.describe_frames, Tracker.describe, StreamPool.describe).  Twelve 64-bit words per slot, 16 slots per frame; the host copies 1.5 KB per
// frame instead of the 2 MB label map.  Every word is an exact integer function of the inputs (include/frtm_hip.h has the full statement):
//   slot of a pixel:  stack: the decoded plane of native_size.hip's rule (per_frame.h);  label map: the index of its id in `ids`, or none
//   label of a pixel: stack: the decoded plane;  label map: its id (listed or not)
//   area, box, sum_x, sum_y; edge = pixels with a 4-neighbour of another label inside the picture; border = pixels on the picture's border
//   conf = sum over the slot's pixels of q(m_slot), mass = sum over ALL pixels of q(m_s);  q(m) = rintf(255 clamp(m, 0, 1)), a NaN gives 0
// All accumulation is integer: a wave's ballot of a row segment gives a slot's counts as popcounts (the coordinate sum and the confidence
// from the bit planes of the lane number and of q), they ride in lanes (lane 4 s + c, three registers: word 4 r + c of slot s), the four waves
// are combined in LDS, then one integer atomic per workgroup and word that changed.  No float atomics: order independent, hence deterministic.
// Loads touch picture samples and the K id bytes only; stores touch the n x 16 x 12 words only.
#include "object_rows.h"     // the table row and its check (shared with mask_runs.hip); MERGE_MAX, merged_offer, merged_plane through per_frame.h
#include <climits>
#include <cstdint>

#define OB_TH 16            // tile: rows (wave tg owns rows tg + 4 i)
#define OB_TW 64            //       columns: lane = column, so a wave's ballot is a row segment
#define OB_LP 68            // bytes per LDS row of the label patch (OB_TW + 2 halo columns, padded)
#define OB_MAX_TILES 127    // tiles per workgroup that the 32-bit sums in registers hold
#define OB_GRID 256         // workgroups per frame, unless OB_MAX_TILES asks for more
#define OB_CELLS 5          // label-patch cells per thread: ceil(18 * 66 / 256)
#define OB_WORDS FRTM_OBJECT_WORDS

static_assert(OB_SLOTS == MERGE_MAX && OB_SLOTS * 4 == 64 && OB_WORDS == 12, "lane 4 s + c holds words c, 4 + c, 8 + c of slot s");

typedef unsigned long long u64;

// words of a slot
enum { OS_AREA, OS_XMIN, OS_YMIN, OS_XMAX, OS_YMAX, OS_SUMX, OS_SUMY, OS_EDGE, OS_BORDER, OS_CONF, OS_MASS, OS_ID };
// q(m) = rintf(255 clamp(m, 0, 1)); fmaxf returns the other operand for a NaN, so a NaN gives 0
__device__ __forceinline__ int ob_q(float m) { return (int)rintf(255.0f * fminf(fmaxf(m, 0.0f), 1.0f)); }

__device__ __forceinline__ int ob_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the sum of the numbers of x's set bits
__device__ __forceinline__ int ob_bit_sum(unsigned x) {
  return __popc(x & 0xAAAAAAAAu) + 2 * __popc(x & 0xCCCCCCCCu) + 4 * __popc(x & 0xF0F0F0F0u) + 8 * __popc(x & 0xFF00FF00u) + 16 * __popc(x & 0xFFFF0000u);
}

// word 4 r + c: 1, 2 are minima, 3, 4 maxima, the others sums
__device__ __forceinline__ int ob_combine(int word, int a, int b) {
  return (word == OS_XMIN || word == OS_YMIN) ? min(a, b) : (word == OS_XMAX || word == OS_YMAX) ? max(a, b) : a + b;
}

// The start of every frame's words: slot s < K = {0, w, h, -1, -1, 0, 0, 0, 0, 0, 0, ids[s]}, every other slot zeros.  One workgroup per frame;
// a frame whose device row is refused gets zeros.
__global__ __launch_bounds__(256) void k_object_begin(const long long* __restrict__ table, long long* __restrict__ out) {
  const long long* row = table + (size_t)OB_ROW * blockIdx.x;
  const int t = threadIdx.x;
  if (t >= OB_SLOTS * OB_WORDS) return;
  const int s = t / OB_WORDS, c = t - s * OB_WORDS;
  long long v = 0;
  if (ob_check(row) == OB_OK && s < (int)row[OW_K]) {
    if (c == OS_XMIN) v = row[OW_W];
    else if (c == OS_YMIN) v = row[OW_H];
    else if (c == OS_XMAX || c == OS_YMAX) v = -1;
    else if (c == OS_ID) v = ((const unsigned char*)row[OW_IDS])[s];
  }
  out[(size_t)blockIdx.x * (OB_SLOTS * OB_WORDS) + t] = v;
}

// One workgroup = up to OB_MAX_TILES OB_TH x OB_TW tiles of one frame (blockIdx.z), one after the other: blockIdx.x, blockIdx.x + gridDim.x, ...
// Every workgroup ends with its atomics on the frame's few words, all in a handful of cache lines, where they are served one after the
// other: measured on a 1080p label map, time = 4.5 us x tiles per workgroup + 0.1 us x workgroups (one tile per workgroup, 2025 of them:
// 125 us; OB_GRID = 256: 63 us, the minimum of the sweep).  So the grid is capped, the sums of a workgroup's tiles stay
// in registers, and a minimum or maximum that would change nothing is not sent.  Per tile:
// (1) The tile's labels with a 1-pixel halo into LDS, coordinates clamped into the picture (a neighbour beyond the border is the pixel itself,
//     so the border makes no edge).  A stack is decoded plane by plane: every thread keeps the running arg-max of its OB_CELLS cells, and the
//     q of the plane over the cells that are the tile's own pixels is the plane's mass (one wave sum per plane).  q(m_slot) of the tile's own
//     pixels goes to LDS beside the labels.
// (2) Row by row -- a row of the tile is one wave's 64 lanes -- per slot present: the ballot of the slot's pixels, and its counts into the
//     lanes that own them.
// After the last tile (3): the four waves combined through LDS; lane 4 s + c of wave 0 adds / minimises / maximises words c, 4 + c, 8 + c of slot s.
__global__ __launch_bounds__(256) void k_describe_frames(const long long* __restrict__ table, long long* __restrict__ out) {
  __shared__ unsigned char lab[(OB_TH + 2) * OB_LP];
  __shared__ unsigned char qv[OB_TH * OB_TW];
  __shared__ unsigned char slot_of[256];
  __shared__ int red[4][3][64];
  const long long* row = table + (size_t)OB_ROW * blockIdx.z;
  if (ob_check(row) != OB_OK) return;                                    // (uniform per workgroup, before any barrier)
  const int h = (int)row[OW_H], w = (int)row[OW_W];
  const int tiles_x = (w + OB_TW - 1) / OB_TW, tiles = tiles_x * ((h + OB_TH - 1) / OB_TH);
  if ((int)blockIdx.x >= tiles) return;                                  // (the grid is sized for the launch's largest frame)
  if ((tiles + (int)gridDim.x - 1) / (int)gridDim.x > OB_MAX_TILES) return;   // (never with the host's grid: the 32-bit sums would not hold)
  const bool stack = row[OW_FORM] == FRTM_OBJECT_MASKS;
  const int K = (int)row[OW_K];
  const unsigned char* ans8 = (const unsigned char*)row[OW_ANS];
  const float* ansf = (const float*)row[OW_ANS];
  const unsigned char* ids = (const unsigned char*)row[OW_IDS];
  const size_t hw = (size_t)h * w;
  const int tid = threadIdx.x, lane = tid & 63, tg = tid >> 6;
  const int c = lane & 3;                                                // lane 4 s + c
  // the lane's three accumulators: words c, 4 + c, 8 + c of slot lane >> 2, over this workgroup's tiles (32 bits hold OB_MAX_TILES tiles:
  // sum_x <= 127 * 1024 * 16383 < 2^31)
  int acc0 = (c == OS_XMIN || c == OS_YMIN) ? INT_MAX : c == OS_XMAX ? -1 : 0;
  int acc1 = c == 0 ? -1 : 0;                                            // y_max | sum_x, sum_y, edge
  int acc2 = 0;                                                          // border, conf, mass, (id)

  if (!stack) {
    int s = OB_NONE;                                                     // id `tid` -> the FIRST slot that lists it (read after the tile's barrier)
    for (int k = K - 1; k >= 0; --k) s = ids[k] == tid ? k : s;
    slot_of[tid] = (unsigned char)s;
  }
  // cell (r, c) of the label patch = the label of pixel (y0 - 1 + r, x0 - 1 + c), coordinates clamped into the picture; thread tid fills cells
  // tid, tid + 256, ... (the last pass repeats the last cell for the threads beyond it: the same value, never counted and never stored twice)
  int cr[OB_CELLS], cc[OB_CELLS], have[OB_CELLS], inner[OB_CELLS];        // have 1: the thread has a j-th cell; inner 1: and it is no halo cell
#pragma unroll
  for (int j = 0; j < OB_CELLS; ++j) {
    const int i = min(tid + 256 * j, (OB_TH + 2) * (OB_TW + 2) - 1);
    cr[j] = i / (OB_TW + 2);
    cc[j] = i - cr[j] * (OB_TW + 2);
    have[j] = tid + 256 * j < (OB_TH + 2) * (OB_TW + 2) ? 1 : 0;
    inner[j] = (have[j] && cr[j] >= 1 && cr[j] <= OB_TH && cc[j] >= 1 && cc[j] <= OB_TW) ? 1 : 0;
  }
  // the workgroup's tiles: blockIdx.x, blockIdx.x + gridDim.x, ... (at most OB_MAX_TILES of them)
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int y0 = (tile / tiles_x) * OB_TH, x0 = (tile - (tile / tiles_x) * tiles_x) * OB_TW;
    // (the flags of the cells and of the lane are compared again in every tile: as masks kept over the loop they cost more scalar registers
    // than there are)
    int c = lane & 3, my_slot = lane >> 2;
    asm volatile("" : "+v"(c), "+v"(my_slot));
#pragma unroll
    for (int j = 0; j < OB_CELLS; ++j) asm volatile("" : "+v"(have[j]), "+v"(inner[j]));
    int pix[OB_CELLS], own[OB_CELLS];                                     // own 1: the cell is a pixel of this tile (and of the picture)
#pragma unroll
    for (int j = 0; j < OB_CELLS; ++j) {
      const int yy = y0 - 1 + cr[j], xx = x0 - 1 + cc[j];
      pix[j] = min(max(yy, 0), h - 1) * w + min(max(xx, 0), w - 1);       // (h w <= 2^28)
      own[j] = inner[j] & (int)(yy < h) & (int)(xx < w);
    }
    if (stack) {
      float best[OB_CELLS], m0[OB_CELLS];
      int arg[OB_CELLS];
#pragma unroll
      for (int j = 0; j < OB_CELLS; ++j) { best[j] = -INFINITY; arg[j] = 0; m0[j] = 0.f; }
      for (int k = 0; k < K; ++k) {
        const float* plane = ansf + (size_t)k * hw;
        int qsum = 0;
#pragma unroll
        for (int j = 0; j < OB_CELLS; ++j) {
          const float m = plane[pix[j]];
          if (k == 0) m0[j] = m;
          merged_offer(m, k, best[j], arg[j]);
          qsum += own[j] * ob_q(m);
        }
        qsum = ob_wave_sum(qsum);
        if (my_slot == k && c == OS_MASS - 8) acc2 += qsum;
      }
#pragma unroll
      for (int j = 0; j < OB_CELLS; ++j) {
        if (have[j]) {
          const int p = merged_plane(arg[j], best[j]);
          lab[cr[j] * OB_LP + cc[j]] = (unsigned char)p;
          // m_slot: the winner's value, or the background plane's when the winner is an object at or below 0.5
          if (own[j]) qv[(cr[j] - 1) * OB_TW + cc[j] - 1] = (unsigned char)ob_q(p == arg[j] ? best[j] : m0[j]);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < OB_CELLS; ++j)
        if (have[j]) lab[cr[j] * OB_LP + cc[j]] = ans8[pix[j]];
    }
    __syncthreads();

    const int x = x0 + lane;
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
      const int ly = tg + 4 * i, y = y0 + ly;
      if (y >= h) break;                                                   // (uniform per wave)
      const bool valid = x < w;
      const unsigned char* p = lab + (ly + 1) * OB_LP + lane + 1;
      const int L = p[0];
      const int slot = stack ? L : slot_of[L];
      const u64 b_edge = __ballot(valid && (p[-OB_LP] != L || p[OB_LP] != L || p[-1] != L || p[1] != L));
      const u64 b_border = __ballot(valid && (y == 0 || y == h - 1 || x == 0 || x == w - 1));
      const int q = stack ? qv[ly * OB_TW + lane] : 0;
      for (int s = 0; s < K; ++s) {
        const u64 b = __ballot(valid && slot == s);
        if (b == 0) continue;                                              // (uniform per wave)
        const int area = __popcll(b);
        // sum of the lane numbers of b's bits, from the bit planes of the lane number
        const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);       // (32-bit masks are literals of the instruction; 64-bit ones occupy registers)
        const int lanes = ob_bit_sum(lo) + ob_bit_sum(hi) + 32 * __popc(hi);
        int conf = 0;                                                      // the sum of q over b's lanes, from the bit planes of q
        if (stack) {
#pragma unroll
          for (int j = 0; j < 8; ++j) conf += __popcll(__ballot(valid && slot == s && ((q >> j) & 1))) << j;
        }
        const int xmin = x0 + (int)__ffsll((unsigned long long)b) - 1, xmax = x0 + 63 - (int)__clzll((long long)b);
        if (my_slot == s) {
          acc0 = c == 0 ? acc0 + area : c == 1 ? min(acc0, xmin) : c == 2 ? min(acc0, y) : max(acc0, xmax);
          acc1 = c == 0 ? max(acc1, y) : c == 1 ? acc1 + area * x0 + lanes : c == 2 ? acc1 + area * y : acc1 + __popcll(b & b_edge);
          acc2 = c == 0 ? acc2 + __popcll(b & b_border) : c == 1 ? acc2 + conf : acc2;
        }
      }
    }
    __syncthreads();                                                     // (the next tile overwrites the patch)
  }

  red[tg][0][lane] = acc0; red[tg][1][lane] = acc1; red[tg][2][lane] = acc2;
  __syncthreads();
  int ce = lane & 3, se = lane >> 2;                                     // (compared here, not held as masks over the tile loop)
  asm volatile("" : "+v"(ce), "+v"(se));
  if (tg != 0 || se >= K) return;
  long long* o = out + ((size_t)blockIdx.z * OB_SLOTS + se) * OB_WORDS;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int word = 4 * r + ce;
    const int v = ob_combine(word, ob_combine(word, red[0][r][lane], red[1][r][lane]), ob_combine(word, red[2][r][lane], red[3][r][lane]));
    if (word == OS_ID) continue;
    // a minimum only falls and a maximum only rises: whatever value the plain load sees, one that v does not improve on needs no atomic
    const long long seen = *(const volatile long long*)(o + word);
    if (word == OS_XMIN || word == OS_YMIN) {
      if (v < seen) atomicMin(o + word, (long long)v);                   // (an empty slot has INT_MAX here: above every start value)
    } else if (word == OS_XMAX || word == OS_YMAX) {
      if (v > seen) atomicMax(o + word, (long long)v);                   // (an empty slot has -1: the start value)
    } else if (v != 0) {
      atomicAdd((u64*)(o + word), (u64)v);                               // (every sum is >= 0: the same bits as a signed add)
    }
  }
}

extern "C" int frtm_describe_frames(const long long* table_host, const long long* table_dev, int n, long long* out, size_t out_words,
                                    frtm_stream_t stream) {
  const char* who = "frtm_describe_frames";
  FRTM_CHECK_ARG(table_host && table_dev, "%s: bad argument (a null table)", who);
  FRTM_CHECK_ARG(out, "%s: bad argument (a null out)", who);
  FRTM_CHECK_ARG(n >= 1 && n <= 65535, "%s: n = %d frames (1 .. 65535)", who, n);
  FRTM_CHECK_ARG(out_words >= (size_t)n * OB_SLOTS * OB_WORDS, "%s: out holds %zu words, %d frames need %zu", who, out_words, n,
                 (size_t)n * OB_SLOTS * OB_WORDS);
  if (ob_check_table(who, table_host, n) != FRTM_OK) return FRTM_ERR_ARG;
  int tiles = 0;                                                         // of the launch's largest frame (<= 256 * 1024)
  for (int i = 0; i < n; ++i) {
    const long long* r = table_host + (size_t)OB_ROW * i;
    tiles = max(tiles, ceil_div((int)r[OW_W], OB_TW) * ceil_div((int)r[OW_H], OB_TH));
  }
  hipStream_t st = (hipStream_t)stream;
  k_object_begin<<<n, 256, 0, st>>>(table_dev, out);
  FRTM_LAUNCH_CHECK();
  dim3 g(max(min(tiles, OB_GRID), ceil_div(tiles, OB_MAX_TILES)), 1, n);
  k_describe_frames<<<g, 256, 0, st>>>(table_dev, out);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}
