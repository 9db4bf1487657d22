// The answer cleaned on the device: every object of a frame split into its connected parts, the parts measured, a keep rule applied and a
// cleaned uint8 label map written -- for all frames of a tick, label maps and merged mask stacks of any sizes, in SIX launches whatever n, the
// sizes and the content (ops.clean_frames, Tracker.clean, StreamPool.clean).  include/frtm_hip.h has the full statement.
//
// Block-based union-find, its phases separated by kernel boundaries (parts_core.h has find, union, the packed maximum and the keep rule; the
// parent array holds pixel indices y w + x, parent[p] <= p, and a union hooks the larger root under the smaller, so a part's root is its
// smallest pixel: its name, whatever the order of the unions):
//   (0) k_parts_begin    the start of every word, status = 0, the packed maxima = 0
//   (1) k_parts_local    a workgroup = one PT_TH x PT_TW tile, a wave = a row, lane = column.  The slots decoded once (and kept in `labels` for
//                        the later passes); row runs from one ballot per row; the runs joined with the row above by union-find in LDS;
//                        parent[p] = the tile's smallest pixel of p's part, area[that pixel] = the part's pixels in the tile, 0 elsewhere
//   (2) k_parts_seam     every pixel on a tile seam joined with its neighbours across the seam, in global memory
//   (3) k_parts_flatten  parent[p] = find(p); a tile-local root that is not the root adds its tile's pixels to the root's area: one atomic
//                        per (tile, part) -- the per-workgroup reduction was made in LDS by (1)
//   (4) k_parts_slots    over the roots: parts, area and max(area << 32 | ~name) per slot, in LDS, then one atomic per workgroup and word
//   (5) k_parts_write    labels, components, kept, kept_area and the largest part's box, from ballots, one atomic per workgroup and word
// Visibility.  gfx950 has eight XCDs with private L2s: a plain load may return a stale word that another workgroup wrote in the same launch.
// In (2) every access to `parent`, and in (3) every access to `parent` and `area`, is a relaxed agent-scope atomic (PtAgent) -- the loads in
// find included; everything else a launch reads was written by an earlier launch.  No grid barrier, no flag a workgroup waits on.
// No loop can spin: parents only decrease, so every find and union makes progress alone, and each carries the trip cap of parts_core.h (the
// length of the array it walks: PT_PIX in LDS, h w in global memory); at the cap the frame's status word is set and the loop left.
// All atomics are vector integer atomics from HIP builtins.
#include "object_rows.h"     // the first 8 words of a row and their check; merged_offer, merged_plane through per_frame.h
#include "parts_core.h"
#include <cstdint>
#include <vector>

#define PT_TH FRTM_PARTS_TILE_H     // tile: rows (wave g owns rows g + 4 i)
#define PT_TW FRTM_PARTS_TILE_W     //       columns: lane = column, so a wave's ballot is a row segment
#define PT_PIX (PT_TH * PT_TW)
#define PT_ROWS (PT_TH / 4)         // rows of a tile per wave
#define PT_ROW FRTM_PARTS_ROW_WORDS
#define PT_WORDS FRTM_PARTS_WORDS
#define PT_PACKED_BYTES (8 * OB_SLOTS)
#define PT_MAX_MIN_AREA (1LL << 28)

static_assert(PT_TW == 64 && PT_TH % 4 == 0 && PT_PIX <= 32768 && PT_WORDS == 12 && PT_ROW == 16, "a row of a tile is one wave");

typedef unsigned long long u64;

// words of a row behind the object row
enum { PW_LABELS = OB_ROW, PW_LABELS_BYTES, PW_COMPS, PW_COMPS_BYTES, PW_WORK, PW_WORK_BYTES, PW_ZERO0, PW_ZERO1 };
// words of a slot
enum { PS_PARTS, PS_KEPT, PS_AREA, PS_KEPT_AREA, PS_LARGEST_AREA, PS_LARGEST_NAME, PS_XMIN, PS_YMIN, PS_XMAX, PS_YMAX, PS_RULED, PS_ID };
// why the second half of a row is refused (after ob_check's reasons)
enum { PT_OK = 0, PT_BAD_TAIL = 100, PT_NULL, PT_NOT_A_SIZE, PT_LABELS_RANGE, PT_OVERLAP, PT_COMPS_ALIGN, PT_COMPS_RANGE, PT_WORK_ALIGN, PT_WORK_RANGE };

// a frame's part of the work buffer: 16 packed words, then parent and area, two int32 per pixel; a multiple of 16 bytes
__host__ __device__ static inline long long pt_frame_work_bytes(long long h, long long w) { return (PT_PACKED_BYTES + 8 * h * w + 15) / 16 * 16; }

// Is row r a frame this launch can clean?  (By the host from its copy, and by every workgroup from the DEVICE table before it touches anything.)
__host__ __device__ static inline int pt_check(const long long* r) {
  const int e = ob_check(r);
  if (e != OB_OK) return e;
  const long long hw = r[OW_H] * r[OW_W];
  if (r[PW_ZERO0] != 0 || r[PW_ZERO1] != 0) return PT_BAD_TAIL;
  if (!r[PW_LABELS] || !r[PW_WORK]) return PT_NULL;
  if (r[PW_LABELS_BYTES] < 0 || r[PW_LABELS_BYTES] > OB_MAXBYTES || r[PW_COMPS_BYTES] < 0 || r[PW_COMPS_BYTES] > OB_MAXBYTES ||
      r[PW_WORK_BYTES] < 0 || r[PW_WORK_BYTES] > OB_MAXBYTES) return PT_NOT_A_SIZE;
  if (r[PW_LABELS_BYTES] < hw) return PT_LABELS_RANGE;
  const long long ans_bytes = r[OW_FORM] == FRTM_OBJECT_MASKS ? 4 * r[OW_K] * hw : hw;
  if (r[PW_LABELS] < r[OW_ANS] + ans_bytes && r[OW_ANS] < r[PW_LABELS] + hw) return PT_OVERLAP;
  if (r[PW_COMPS]) {
    if (r[PW_COMPS] & 3) return PT_COMPS_ALIGN;
    if (r[PW_COMPS_BYTES] < 4 * hw) return PT_COMPS_RANGE;
  }
  if (r[PW_WORK] & 15) return PT_WORK_ALIGN;
  if (r[PW_WORK_BYTES] < pt_frame_work_bytes(r[OW_H], r[OW_W])) return PT_WORK_RANGE;
  return PT_OK;
}

// global memory that other workgroups write in the same launch: relaxed agent-scope atomics only
struct PtAgent {
  __device__ __forceinline__ static int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ static int fetch_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// LDS that the other waves of the workgroup write between two barriers
struct PtLds {
  __device__ __forceinline__ static int load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ static int fetch_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};

struct PtFrame {
  int h, w, K, tiles_x, tiles;
  bool stack;
  const unsigned char* ans8;
  const float* ansf;
  const unsigned char* ids;
  unsigned char* labels;
  int* comps;
  u64* packed;
  int* parent;
  int* area;
};

// Frame f of the DEVICE table, when this launch can clean it
__device__ __forceinline__ bool pt_frame(const long long* table, int f, PtFrame& F) {
  const long long* row = table + (size_t)PT_ROW * f;
  if (pt_check(row) != PT_OK) return false;
  F.h = (int)row[OW_H]; F.w = (int)row[OW_W]; F.K = (int)row[OW_K];
  F.tiles_x = (F.w + PT_TW - 1) / PT_TW;
  F.tiles = F.tiles_x * ((F.h + PT_TH - 1) / PT_TH);
  F.stack = row[OW_FORM] == FRTM_OBJECT_MASKS;
  F.ans8 = (const unsigned char*)row[OW_ANS];
  F.ansf = (const float*)row[OW_ANS];
  F.ids = (const unsigned char*)row[OW_IDS];
  F.labels = (unsigned char*)row[PW_LABELS];
  F.comps = (int*)row[PW_COMPS];
  F.packed = (u64*)row[PW_WORK];
  F.parent = (int*)(row[PW_WORK] + PT_PACKED_BYTES);
  F.area = F.parent + (size_t)F.h * F.w;
  return true;
}

__device__ __forceinline__ void pt_gave_up(long long* status, int f, int bit) { atomicOr((u64*)status + f, (u64)bit); }

// (0): one workgroup per frame.  Slot s < K = {0, 0, 0, 0, 0, -1, w, h, -1, -1, ruled, ids[s]}, every other slot zeros; a frame whose device row
// is refused gets zeros and nothing else.
__global__ __launch_bounds__(256) void k_parts_begin(const long long* __restrict__ table, int fill, long long* __restrict__ words,
                                                     long long* __restrict__ status) {
  const int f = blockIdx.x, t = threadIdx.x;
  const long long* row = table + (size_t)PT_ROW * f;
  const bool good = pt_check(row) == PT_OK;
  if (t < OB_SLOTS * PT_WORDS) {
    const int s = t / PT_WORDS, c = t - s * PT_WORDS;
    long long v = 0;
    if (good && s < (int)row[OW_K]) {
      const int id = ((const unsigned char*)row[OW_IDS])[s];
      if (c == PS_XMIN) v = row[OW_W];
      else if (c == PS_YMIN) v = row[OW_H];
      else if (c == PS_XMAX || c == PS_YMAX || c == PS_LARGEST_NAME) v = -1;
      else if (c == PS_RULED) v = id != fill;
      else if (c == PS_ID) v = id;
    }
    words[(size_t)f * (OB_SLOTS * PT_WORDS) + t] = v;
  } else if (t == OB_SLOTS * PT_WORDS) {
    status[f] = 0;
  } else if (good && t - OB_SLOTS * PT_WORDS - 1 < OB_SLOTS) {
    ((u64*)row[PW_WORK])[t - OB_SLOTS * PT_WORDS - 1] = 0;
  }
}

// id -> the FIRST slot that lists it (label maps; read after a barrier)
__device__ __forceinline__ void pt_slot_table(const PtFrame& F, unsigned char* slot_of, int tid) {
  if (F.stack) return;
  int s = OB_NONE;
  for (int k = F.K - 1; k >= 0; --k) s = F.ids[k] == tid ? k : s;
  slot_of[tid] = (unsigned char)s;
}

// (1): blockIdx = (tile, frame); the grid is sized for the launch's largest frame.
__global__ __launch_bounds__(256) void k_parts_local(const long long* __restrict__ table, int conn8, long long* __restrict__ status) {
  __shared__ unsigned char sl[PT_PIX];      // the slot of every pixel of the tile; OB_NONE: none, or outside the picture
  __shared__ int lab[PT_PIX];               // the union-find over the tile: local indices ly * PT_TW + lx (the order of the global ones)
  __shared__ int cnt[PT_PIX];               // pixels of a tile-local part, at its root
  __shared__ int rt[PT_PIX];                // the root of a run, at the run's first pixel
  __shared__ unsigned char st[PT_PIX];      // the lane that starts the pixel's run
  __shared__ unsigned char ln[PT_PIX];      // the length of the run that starts at the pixel
  __shared__ unsigned char slot_of[256];
  const int f = blockIdx.y;
  PtFrame F;
  if (!pt_frame(table, f, F)) return;                                    // (uniform per workgroup, before any barrier)
  if ((int)blockIdx.x >= F.tiles) return;
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int h = F.h, w = F.w, K = F.K;
  const int y0 = ((int)blockIdx.x / F.tiles_x) * PT_TH, x0 = ((int)blockIdx.x % F.tiles_x) * PT_TW;
  const int x = x0 + lane, xc = min(x, w - 1);
  const size_t hw = (size_t)h * w;
  pt_slot_table(F, slot_of, tid);
  if (!F.stack) __syncthreads();

  {
    int slot[PT_ROWS];
    if (F.stack) {
      float best[PT_ROWS];
#pragma unroll
      for (int i = 0; i < PT_ROWS; ++i) { best[i] = -INFINITY; slot[i] = 0; }
      for (int k = 0; k < K; ++k) {
        const float* plane = F.ansf + (size_t)k * hw;
        float m[PT_ROWS];
#pragma unroll
        for (int i = 0; i < PT_ROWS; ++i) m[i] = plane[(size_t)min(y0 + g + 4 * i, h - 1) * w + xc];
#pragma unroll
        for (int i = 0; i < PT_ROWS; ++i) merged_offer(m[i], k, best[i], slot[i]);
      }
#pragma unroll
      for (int i = 0; i < PT_ROWS; ++i) slot[i] = merged_plane(slot[i], best[i]);
    } else {
      unsigned char L[PT_ROWS];
#pragma unroll
      for (int i = 0; i < PT_ROWS; ++i) L[i] = F.ans8[(size_t)min(y0 + g + 4 * i, h - 1) * w + xc];
#pragma unroll
      for (int i = 0; i < PT_ROWS; ++i) slot[i] = slot_of[L[i]];
    }
#pragma unroll
    for (int i = 0; i < PT_ROWS; ++i) sl[(g + 4 * i) * PT_TW + lane] = (unsigned char)((y0 + g + 4 * i >= h || x >= w) ? OB_NONE : slot[i]);
  }
  // row runs (a wave reads back the rows it wrote): a lane starts a run when its slot differs from its left neighbour's; every pixel begins
  // as its run's first pixel.  The loops over the rows are not unrolled: what a row needs later is in LDS, not in registers.
#pragma unroll 1
  for (int i = 0; i < PT_ROWS; ++i) {
    const int me = (g + 4 * i) * PT_TW + lane;
    const int s = sl[me];
    const int left = __shfl_up(s, 1, 64);
    const u64 B = __ballot(lane == 0 || left != s);
    const int start = 63 - (int)__clzll((long long)(B & (~0ULL >> (63 - lane))));
    const u64 next = lane < 63 ? B >> (lane + 1) : 0;
    st[me] = (unsigned char)start;
    ln[me] = (unsigned char)(next ? (int)__ffsll((unsigned long long)next) : 64 - lane);   // 1 .. 64: of the run that starts here
    lab[me] = me - lane + start;
    cnt[me] = 0;
  }
  __syncthreads();
  // the runs joined with the row above.  With q the row above: N joins when the pixel starts its run or its left neighbour's N is of another
  // slot (else the left neighbour, of the same run, has joined the same two runs); NW only matters at a run's first pixel, NE at its last.
  bool gave_up = false;
#pragma unroll 1
  for (int i = 0; i < PT_ROWS; ++i) {
    const int ly = g + 4 * i, me = ly * PT_TW + lane, up = me - PT_TW;
    const int s = sl[me];
    if (ly == 0 || s == OB_NONE) continue;
    const bool first = st[me] == lane, last = lane == 63 || sl[me + 1] != s;
    if (sl[up] == s && (first || sl[up - 1] != s)) pt_union<PtLds>(lab, me, up, PT_PIX, &gave_up);
    if (conn8) {
      if (first && lane > 0 && sl[up - 1] == s) pt_union<PtLds>(lab, me, up - 1, PT_PIX, &gave_up);
      if (last && lane < 63 && sl[up + 1] == s) pt_union<PtLds>(lab, me, up + 1, PT_PIX, &gave_up);
    }
  }
  __syncthreads();
  // every run's root, found by its first lane and left in rt at the run's first pixel; the run's pixels counted at the root
#pragma unroll 1
  for (int i = 0; i < PT_ROWS; ++i) {
    const int me = (g + 4 * i) * PT_TW + lane;
    if (sl[me] == OB_NONE || st[me] != lane) continue;
    const int r = pt_find<PtLds>(lab, me, PT_PIX, &gave_up);            // (other waves shorten paths of lab meanwhile)
    rt[me] = r;
    atomicAdd(&cnt[r], (int)ln[me]);
  }
  __syncthreads();
#pragma unroll 1
  for (int i = 0; i < PT_ROWS; ++i) {
    const int ly = g + 4 * i, y = y0 + ly, me = ly * PT_TW + lane;
    if (y >= h || x >= w) continue;
    const size_t p = (size_t)y * w + x;
    const int s = sl[me];
    F.labels[p] = (unsigned char)s;
    const bool has = s != OB_NONE;
    const int r = has ? rt[me - lane + st[me]] : 0;
    F.parent[p] = has ? (y0 + (r >> 6)) * w + x0 + (r & 63) : -1;
    F.area[p] = (has && r == me) ? cnt[me] : 0;
  }
  if (gave_up) pt_gave_up(status, f, PT_GAVE_UP_LOCAL);
}

// (2): blockIdx = (tile, frame), two waves.  Wave 0: the tile's top row, joined with the row above (N; NW and NE at 8) and, at the tile's
// first column, with W.  Wave 1, lanes 0 .. 31: the first column below the corner (W; NW at 8); lanes 32 .. 63: the last column below the
// corner (NE at 8).  Every pair of neighbours in different tiles is {p, one of W, NW, N, NE of p} for exactly one p on a seam.
__device__ __forceinline__ void pt_join(const PtFrame& F, int p, int s, int qy, int qx, bool* gave_up) {
  const int q = qy * F.w + qx;
  if (F.labels[q] == s) pt_union<PtAgent>(F.parent, p, q, F.h * F.w, gave_up);
}

__global__ __launch_bounds__(128) void k_parts_seam(const long long* table, int conn8, long long* __restrict__ status) {
  const int f = blockIdx.y;
  PtFrame F;
  if (!pt_frame(table, f, F)) return;
  if ((int)blockIdx.x >= F.tiles) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = F.h, w = F.w;
  const int y0 = ((int)blockIdx.x / F.tiles_x) * PT_TH, x0 = ((int)blockIdx.x % F.tiles_x) * PT_TW;
  int ly, lx;
  if (wave == 0) { ly = 0; lx = lane; }
  else { ly = 1 + (lane & 31); lx = lane < 32 ? 0 : PT_TW - 1; }
  const int y = y0 + ly, x = x0 + lx;
  if (ly >= PT_TH || y >= h || x >= w) return;
  const int p = y * w + x;                                               // (h w <= 2^28)
  const int s = F.labels[p];
  if (s == OB_NONE) return;
  bool gave_up = false;
  if (ly == 0) {
    if (y > 0) {
      pt_join(F, p, s, y - 1, x, &gave_up);
      if (conn8 && x > 0) pt_join(F, p, s, y - 1, x - 1, &gave_up);
      if (conn8 && x < w - 1) pt_join(F, p, s, y - 1, x + 1, &gave_up);
    }
    if (lx == 0 && x > 0) pt_join(F, p, s, y, x - 1, &gave_up);
  } else if (lx == 0) {
    if (x > 0) {
      pt_join(F, p, s, y, x - 1, &gave_up);
      if (conn8) pt_join(F, p, s, y - 1, x - 1, &gave_up);
    }
  } else if (conn8 && x < w - 1) {
    pt_join(F, p, s, y - 1, x + 1, &gave_up);
  }
  if (gave_up) pt_gave_up(status, f, PT_GAVE_UP_SEAM);
}

// (3): blockIdx = (tile, frame).  parent[p] = the root (a store other walks may read: it only shortens them); a tile-local root that is not
// the root adds its tile's pixels to the root's area.  Nobody adds to the area of a pixel that is not a root, so what such a pixel reads
// there is the count (1) left.
__global__ __launch_bounds__(256) void k_parts_flatten(const long long* table, long long* __restrict__ status) {
  const int f = blockIdx.y;
  PtFrame F;
  if (!pt_frame(table, f, F)) return;
  if ((int)blockIdx.x >= F.tiles) return;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int h = F.h, w = F.w;
  const int y0 = ((int)blockIdx.x / F.tiles_x) * PT_TH, x = ((int)blockIdx.x % F.tiles_x) * PT_TW + lane;
  bool gave_up = false;
  for (int i = 0; i < PT_ROWS; ++i) {
    const int y = y0 + g + 4 * i;
    if (y >= h || x >= w) continue;
    const int p = y * w + x;
    if (F.labels[p] == OB_NONE) continue;
    const int r = pt_find<PtAgent>(F.parent, p, h * w, &gave_up);
    if (r == p) continue;
    __hip_atomic_store(F.parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int mine = __hip_atomic_load(F.area + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (mine > 0) __hip_atomic_fetch_add(F.area + r, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (gave_up) pt_gave_up(status, f, PT_GAVE_UP_FLATTEN);
}

// (4): blockIdx = (tile, frame).  Over the tile's roots: parts, area and the packed maximum per slot, in LDS; then one atomic per word.
__global__ __launch_bounds__(256) void k_parts_slots(const long long* __restrict__ table, long long* __restrict__ words) {
  __shared__ unsigned int parts[OB_SLOTS], pixels[OB_SLOTS];             // (the areas of distinct parts sum to at most h w <= 2^28)
  __shared__ u64 big[OB_SLOTS];
  const int f = blockIdx.y;
  PtFrame F;
  if (!pt_frame(table, f, F)) return;
  if ((int)blockIdx.x >= F.tiles) return;
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int h = F.h, w = F.w;
  const int y0 = ((int)blockIdx.x / F.tiles_x) * PT_TH, x = ((int)blockIdx.x % F.tiles_x) * PT_TW + lane;
  if (tid < OB_SLOTS) { parts[tid] = 0; pixels[tid] = 0; big[tid] = 0; }
  __syncthreads();
  for (int i = 0; i < PT_ROWS; ++i) {
    const int y = y0 + g + 4 * i;
    if (y >= h || x >= w) continue;
    const int p = y * w + x;
    const int s = F.labels[p];
    if (s >= F.K || F.parent[p] != p) continue;
    const int a = F.area[p];
    atomicAdd(&parts[s], 1u);
    atomicAdd(&pixels[s], (unsigned int)a);
    atomicMax(&big[s], pt_pack(a, p));
  }
  __syncthreads();
  if (tid < F.K && parts[tid] != 0) {
    long long* o = words + ((size_t)f * OB_SLOTS + tid) * PT_WORDS;
    atomicAdd((u64*)(o + PS_PARTS), (u64)parts[tid]);
    atomicAdd((u64*)(o + PS_AREA), (u64)pixels[tid]);
    atomicMax(F.packed + tid, big[tid]);
  }
}

// (5): blockIdx = (tile, frame).  Every pixel: its part's name and area, the rule, the cleaned byte and the name.  Per row -- one wave -- and
// slot present, ballots give the kept pixels, the kept roots and the extent of the largest part; lane s holds slot s's sums.  Then the four
// waves combined through LDS and one atomic per workgroup and word that changed.  Tile 0 also writes the largest part's area and name.
__global__ __launch_bounds__(256) void k_parts_write(const long long* __restrict__ table, long long min_area, int largest_only, int fill,
                                                     long long* __restrict__ words) {
  __shared__ int big_name[OB_SLOTS], big_area[OB_SLOTS];
  __shared__ unsigned char id_of[OB_SLOTS], ruled[OB_SLOTS];
  __shared__ int red[4][6][OB_SLOTS];
  const int f = blockIdx.y;
  PtFrame F;
  if (!pt_frame(table, f, F)) return;
  if ((int)blockIdx.x >= F.tiles) return;
  const int tid = threadIdx.x, lane = tid & 63, g = tid >> 6;
  const int h = F.h, w = F.w, K = F.K;
  const int y0 = ((int)blockIdx.x / F.tiles_x) * PT_TH, x0 = ((int)blockIdx.x % F.tiles_x) * PT_TW, x = x0 + lane;
  if (tid < OB_SLOTS) {
    const u64 v = tid < K ? F.packed[tid] : 0;
    big_name[tid] = pt_packed_name(v);
    big_area[tid] = pt_packed_area(v);
    id_of[tid] = tid < K ? F.ids[tid] : 0;
    ruled[tid] = tid < K && id_of[tid] != fill;
  }
  __syncthreads();
  int kept_parts = 0, kept_pixels = 0, bx0 = w, by0 = h, bx1 = -1, by1 = -1;   // of slot `lane`
  for (int i = 0; i < PT_ROWS; ++i) {
    const int y = y0 + g + 4 * i;
    if (y >= h) break;                                                   // (uniform per wave)
    const bool valid = x < w;
    const int p = y * w + min(x, w - 1);
    int s = F.labels[p];
    bool keep = false, root = false, in_big = false;
    if (valid && s < K) {
      const int r = F.parent[p];
      keep = pt_keep(ruled[s], F.area[r], r, big_name[s], min_area, largest_only != 0);
      root = r == p;
      in_big = r == big_name[s];
      F.labels[p] = keep ? id_of[s] : (unsigned char)fill;
      if (F.comps) F.comps[p] = r;
    } else if (valid) {
      F.labels[p] = F.ans8[p];                                           // (a label map's pixel whose id is not listed: a stack has none)
      if (F.comps) F.comps[p] = -1;
    }
    if (!valid) s = OB_NONE;
    for (int k = 0; k < K; ++k) {
      const u64 b = __ballot(s == k);
      if (b == 0) continue;                                              // (uniform per wave)
      const u64 bk = __ballot(s == k && keep), br = __ballot(s == k && keep && root), bb = __ballot(s == k && in_big);
      if (lane == k) {
        kept_pixels += __popcll(bk);
        kept_parts += __popcll(br);
        if (bb) {
          bx0 = min(bx0, x0 + (int)__ffsll((unsigned long long)bb) - 1);
          bx1 = max(bx1, x0 + 63 - (int)__clzll((long long)bb));
          by0 = min(by0, y);
          by1 = max(by1, y);
        }
      }
    }
  }
  if (lane < OB_SLOTS) {
    red[g][0][lane] = kept_parts; red[g][1][lane] = kept_pixels;
    red[g][2][lane] = bx0; red[g][3][lane] = by0; red[g][4][lane] = bx1; red[g][5][lane] = by1;
  }
  __syncthreads();
  if (tid >= K) return;
  long long* o = words + ((size_t)f * OB_SLOTS + tid) * PT_WORDS;
  kept_parts = red[0][0][tid] + red[1][0][tid] + red[2][0][tid] + red[3][0][tid];
  kept_pixels = red[0][1][tid] + red[1][1][tid] + red[2][1][tid] + red[3][1][tid];
  bx0 = min(min(red[0][2][tid], red[1][2][tid]), min(red[2][2][tid], red[3][2][tid]));
  by0 = min(min(red[0][3][tid], red[1][3][tid]), min(red[2][3][tid], red[3][3][tid]));
  bx1 = max(max(red[0][4][tid], red[1][4][tid]), max(red[2][4][tid], red[3][4][tid]));
  by1 = max(max(red[0][5][tid], red[1][5][tid]), max(red[2][5][tid], red[3][5][tid]));
  if (kept_parts) atomicAdd((u64*)(o + PS_KEPT), (u64)kept_parts);
  if (kept_pixels) atomicAdd((u64*)(o + PS_KEPT_AREA), (u64)kept_pixels);
  if (bx1 >= 0) {                                                        // (the start values are w, h, -1, -1: an empty extent changes nothing)
    atomicMin(o + PS_XMIN, (long long)bx0);
    atomicMin(o + PS_YMIN, (long long)by0);
    atomicMax(o + PS_XMAX, (long long)bx1);
    atomicMax(o + PS_YMAX, (long long)by1);
  }
  if (blockIdx.x == 0) {                                                 // (no other workgroup touches these two words in this launch)
    o[PS_LARGEST_AREA] = big_area[tid];
    o[PS_LARGEST_NAME] = big_name[tid];
  }
}

// The host's pass over its copy of the table: the first 8 words by ob_check_table (on a compact copy of the rows up to the refused one, made
// on that path only), then the rest.  `outputs` false: the first 8 words only (frtm_clean_work_bytes, before the outputs exist).
static int pt_check_table(const char* who, const long long* table_host, int n, bool outputs) {
  FRTM_CHECK_ARG(table_host, "%s: bad argument (a null table)", who);
  FRTM_CHECK_ARG(n >= 1 && n <= 65535, "%s: n = %d frames (1 .. 65535)", who, n);
  for (int i = 0; i < n; ++i) {
    const long long* r = table_host + (size_t)PT_ROW * i;
    if (ob_check(r) != OB_OK) {                                          // (rows 0 .. i - 1 pass: the message names frame i)
      std::vector<long long> first((size_t)OB_ROW * (i + 1));
      for (int k = 0; k <= i; ++k)
        for (int j = 0; j < OB_ROW; ++j) first[(size_t)OB_ROW * k + j] = table_host[(size_t)PT_ROW * k + j];
      return ob_check_table(who, first.data(), i + 1);
    }
    if (!outputs) continue;
    const long long hw = r[OW_H] * r[OW_W];
    switch (pt_check(r)) {
      case PT_OK: break;
      case PT_BAD_TAIL: FRTM_CHECK_ARG(false, "%s: frame %d has last words %lld, %lld (0, 0)", who, i, r[PW_ZERO0], r[PW_ZERO1]);
      case PT_NULL: FRTM_CHECK_ARG(false, "%s: frame %d has a null address (labels %#llx, work %#llx)", who, i, r[PW_LABELS], r[PW_WORK]);
      case PT_NOT_A_SIZE:
        FRTM_CHECK_ARG(false, "%s: frame %d: labels_bytes %lld, components_bytes %lld or work_bytes %lld is not a size", who, i,
                       r[PW_LABELS_BYTES], r[PW_COMPS_BYTES], r[PW_WORK_BYTES]);
      case PT_LABELS_RANGE:
        FRTM_CHECK_ARG(false, "%s: frame %d's cleaned map (%lld bytes) leaves its %lld-byte buffer", who, i, hw, r[PW_LABELS_BYTES]);
      case PT_OVERLAP: FRTM_CHECK_ARG(false, "%s: frame %d's cleaned map at %#llx overlaps its answer at %#llx", who, i, r[PW_LABELS], r[OW_ANS]);
      case PT_COMPS_ALIGN: FRTM_CHECK_ARG(false, "%s: frame %d's component map at %#llx is not 4-byte aligned", who, i, r[PW_COMPS]);
      case PT_COMPS_RANGE:
        FRTM_CHECK_ARG(false, "%s: frame %d's component map (%lld bytes) leaves its %lld-byte buffer", who, i, 4 * hw, r[PW_COMPS_BYTES]);
      case PT_WORK_ALIGN: FRTM_CHECK_ARG(false, "%s: frame %d's work at %#llx is not 16-byte aligned", who, i, r[PW_WORK]);
      default:
        FRTM_CHECK_ARG(false, "%s: frame %d's work holds %lld bytes, it needs %lld", who, i, r[PW_WORK_BYTES], pt_frame_work_bytes(r[OW_H], r[OW_W]));
    }
  }
  return FRTM_OK;
}

extern "C" size_t frtm_clean_work_bytes(const long long* table_host, int n) {
  if (pt_check_table("frtm_clean_work_bytes", table_host, n, false) != FRTM_OK) return 0;
  size_t total = 0;
  for (int i = 0; i < n; ++i) total += (size_t)pt_frame_work_bytes(table_host[(size_t)PT_ROW * i + OW_H], table_host[(size_t)PT_ROW * i + OW_W]);
  return total;
}

extern "C" int frtm_clean_frames(const long long* table_host, const long long* table_dev, int n, int connectivity, long long min_area,
                                 int largest_only, int fill, long long* words, size_t word_count, long long* status, size_t status_count,
                                 frtm_stream_t stream) {
  const char* who = "frtm_clean_frames";
  FRTM_CHECK_ARG(table_host && table_dev, "%s: bad argument (a null table)", who);
  FRTM_CHECK_ARG(words && status, "%s: bad argument (a null words or status)", who);
  FRTM_CHECK_ARG(!((uintptr_t)words & 7) && !((uintptr_t)status & 7), "%s: words and status are 8-byte aligned (got %p, %p)", who, (void*)words,
                 (void*)status);
  FRTM_CHECK_ARG(connectivity == 4 || connectivity == 8, "%s: connectivity = %d (4 or 8)", who, connectivity);
  FRTM_CHECK_ARG(min_area >= 1 && min_area <= PT_MAX_MIN_AREA, "%s: min_area = %lld (1 .. 2^28)", who, min_area);
  FRTM_CHECK_ARG(largest_only == 0 || largest_only == 1, "%s: largest_only = %d (0 or 1)", who, largest_only);
  FRTM_CHECK_ARG(fill >= 0 && fill <= 255, "%s: fill = %d (0 .. 255)", who, fill);
  if (pt_check_table(who, table_host, n, true) != FRTM_OK) return FRTM_ERR_ARG;
  FRTM_CHECK_ARG(word_count >= (size_t)n * OB_SLOTS * PT_WORDS, "%s: words holds %zu words, %d frames need %zu", who, word_count, n,
                 (size_t)n * OB_SLOTS * PT_WORDS);
  FRTM_CHECK_ARG(status_count >= (size_t)n, "%s: status holds %zu words, %d frames need %d", who, status_count, n, n);
  int tiles = 0;                                                         // of the launch's largest frame (<= 256 * 512)
  for (int i = 0; i < n; ++i) {
    const long long* r = table_host + (size_t)PT_ROW * i;
    tiles = max(tiles, ceil_div((int)r[OW_W], PT_TW) * ceil_div((int)r[OW_H], PT_TH));
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(tiles, n);
  const int conn8 = connectivity == 8;
  k_parts_begin<<<n, 256, 0, st>>>(table_dev, fill, words, status);
  FRTM_LAUNCH_CHECK();
  k_parts_local<<<grid, 256, 0, st>>>(table_dev, conn8, status);
  FRTM_LAUNCH_CHECK();
  k_parts_seam<<<grid, 128, 0, st>>>(table_dev, conn8, status);
  FRTM_LAUNCH_CHECK();
  k_parts_flatten<<<grid, 256, 0, st>>>(table_dev, status);
  FRTM_LAUNCH_CHECK();
  k_parts_slots<<<grid, 256, 0, st>>>(table_dev, words);
  FRTM_LAUNCH_CHECK();
  k_parts_write<<<grid, 256, 0, st>>>(table_dev, min_area, largest_only, fill, words);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}
