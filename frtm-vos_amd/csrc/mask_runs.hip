// The tracked masks in the form every consumer of segmentation reads, coded on the device: per object of a frame its binary mask as COCO
// run lengths -- scanned column-major (p = x h + y), alternating runs starting with a run of zeros -- for all frames of a tick, label maps and
// merged mask stacks of any sizes, in FOUR launches whatever n, the sizes and the content (ops.encode_frames, Tracker.encode,
// StreamPool.encode).  The host copies a few KB per object instead of the 2 MB label map.  include/frtm_hip.h has the full statement.
//
// A pixel p starts a new run of slot s exactly when b_s(p) != b_s(p - 1), with b_s(-1) = 0: such a p is a BOUNDARY of s.  With Q_0 < Q_1 < ...
// the B boundaries of a slot, its list is Q_0, Q_1 - Q_0, ..., Q_{B-1} - Q_{B-2}, N - Q_{B-1} (B + 1 entries; [N] when there is none; Q_0 = 0
// when b_s(0) = 1, which gives the leading 0).  p - 1 of a pixel in row 0 is the last row of the previous column, and a change of the slot
// from a to b at p is a boundary of a and of b only: one comparison with the vertical neighbour per pixel, whatever K.
// The order comes from a CELL: (frame, slot, column, segment of MR_SEG rows), in that order -- which is increasing p within a slot.
//   (1) k_runs_walk<false>  a wave = 64 columns x one segment, lane = column, rows top down (loads stay row-major and coalesced): per cell
//                           its boundaries, its pixels and its last boundary                                   -> work
//   (2) k_runs_scan         one workgroup per (frame, slot): the exclusive sum of the boundaries and the exclusive maximum of the last
//                           boundary over the slot's cells, in place; the slot's count, area and id            -> heads
//   (3) k_runs_heads        one workgroup: the exclusive sum of the counts over all (frame, slot)             -> heads' offsets, and every
//                           list's last element N - Q_{B-1}
//   (4) k_runs_walk<true>   the walk of (1) again; boundary j of a cell is element offset + first(cell) + j: p minus the boundary before it
// No atomics and no float arithmetic after the decode: every word is a function of the inputs alone.  Element j of the concatenation is
// stored iff j < run_capacity.  Loads touch picture samples and the K id bytes only (and the table, heads and work).
#include "object_rows.h"     // the table row and its check (shared with object_report.hip); merged_offer, merged_plane through per_frame.h
#include <cstdint>

#define MR_TW 64            // columns of a wave: lane = column
#define MR_SEG 64           // rows of a cell
#define MR_CHUNK 8          // rows whose loads are issued together
#define MR_HEAD FRTM_RUNS_HEAD_WORDS
#define MR_MAXCAP (1ULL << 40)

static_assert(MR_HEAD == 4 && MR_SEG < (1 << 15) && MR_SEG % MR_CHUNK == 0, "a cell's boundaries and pixels share one 32-bit word");

typedef unsigned int u32;
typedef unsigned long long u64;

// words of a head
enum { RH_COUNT, RH_OFFSET, RH_AREA, RH_ID };

// cells of a frame (<= 16 * 16384 * 256 = 2^26)
__host__ __device__ static inline long long mr_cells(const long long* r) { return r[OW_K] * r[OW_W] * ((r[OW_H] + MR_SEG - 1) / MR_SEG); }

// work: n x 16 last boundaries, then n x `stride` cells of two words, `stride` the cells of the launch's largest frame
__host__ __device__ static inline size_t mr_work_bytes(int n, long long stride) { return sizeof(u32) * ((size_t)n * OB_SLOTS + 2 * (size_t)n * (size_t)stride); }

struct MrFrame {
  int h, w, K, segs, tiles_x;
  bool stack;
  const unsigned char* ans8;
  const float* ansf;
  const unsigned char* ids;
};

// Frame f of the DEVICE table, when this launch can code it: the row passes ob_check and its cells fit the stride the host sized work for.
__device__ __forceinline__ bool mr_frame(const long long* __restrict__ table, int f, long long stride, MrFrame& F) {
  const long long* row = table + (size_t)OB_ROW * f;
  if (ob_check(row) != OB_OK || mr_cells(row) > stride) return false;
  F.h = (int)row[OW_H]; F.w = (int)row[OW_W]; F.K = (int)row[OW_K];
  F.segs = (F.h + MR_SEG - 1) / MR_SEG;
  F.tiles_x = (F.w + MR_TW - 1) / MR_TW;
  F.stack = row[OW_FORM] == FRTM_OBJECT_MASKS;
  F.ans8 = (const unsigned char*)row[OW_ANS];
  F.ansf = (const float*)row[OW_ANS];
  F.ids = (const unsigned char*)row[OW_IDS];
  return true;
}

// the slot of pixel (y, x) (inside the picture)
__device__ __forceinline__ int mr_slot_at(const MrFrame& F, const unsigned char* slot_of, int y, int x) {
  const int pix = y * F.w + x;                                           // (h w <= 2^28)
  if (!F.stack) return slot_of[F.ans8[pix]];
  const size_t hw = (size_t)F.h * F.w;
  float best = -INFINITY;
  int arg = 0;
  for (int k = 0; k < F.K; ++k) merged_offer(F.ansf[(size_t)k * hw + pix], k, best, arg);
  return merged_plane(arg, best);
}

// One wave = columns x0 .. x0 + 63 of rows y0 .. y0 + MR_SEG - 1 (segment g) of frame f; a[s * 64 + lane], b[s * 64 + lane]: this lane's two
// words of slot s, in LDS that no other wave touches (bank = lane % 32 whatever s: no conflict).
//   EMIT false: a = boundaries | pixels << 16 of the cell, b = its last boundary (0: none, or position 0 -- the same for a difference)
//   EMIT true:  a = the index of the cell's next boundary in the slot's list, b = the boundary before it
template <bool EMIT>
__device__ __forceinline__ void mr_walk(const MrFrame& F, const unsigned char* slot_of, int x0, int g, int lane, u32* __restrict__ a,
                                        u32* __restrict__ b, uint2* __restrict__ cells, const u64* __restrict__ base,
                                        u32* __restrict__ runs, u64 capacity) {
  const int h = F.h, w = F.w, K = F.K;
  const int x = x0 + lane, xc = min(x, w - 1);                           // (a lane beyond the picture loads its last column and counts nothing)
  const bool valid = x < w;
  const int y0 = g * MR_SEG, y1 = min(y0 + MR_SEG, h);
  const size_t hw = (size_t)h * w;
  for (int s = 0; s < K; ++s) {
    uint2 v = make_uint2(0u, 0u);
    if (EMIT && valid) v = cells[((size_t)s * w + x) * F.segs + g];
    a[s * 64 + lane] = v.x;
    b[s * 64 + lane] = v.y;
  }
  // p - 1: the row above, or the last row of the previous column; pixel 0 follows a virtual pixel without a slot
  int prev = OB_NONE;
  if (valid && (y0 > 0 || x > 0)) prev = y0 > 0 ? mr_slot_at(F, slot_of, y0 - 1, x) : mr_slot_at(F, slot_of, h - 1, x - 1);
  for (int yb = y0; yb < y1; yb += MR_CHUNK) {
    int slot[MR_CHUNK];
    if (F.stack) {
      float best[MR_CHUNK];
#pragma unroll
      for (int r = 0; r < MR_CHUNK; ++r) { best[r] = -INFINITY; slot[r] = 0; }
      for (int k = 0; k < K; ++k) {
        const float* plane = F.ansf + (size_t)k * hw;
        float m[MR_CHUNK];
#pragma unroll
        for (int r = 0; r < MR_CHUNK; ++r) m[r] = plane[min(yb + r, h - 1) * w + xc];
#pragma unroll
        for (int r = 0; r < MR_CHUNK; ++r) merged_offer(m[r], k, best[r], slot[r]);
      }
#pragma unroll
      for (int r = 0; r < MR_CHUNK; ++r) slot[r] = merged_plane(slot[r], best[r]);
    } else {
      unsigned char L[MR_CHUNK];
#pragma unroll
      for (int r = 0; r < MR_CHUNK; ++r) L[r] = F.ans8[min(yb + r, h - 1) * w + xc];
#pragma unroll
      for (int r = 0; r < MR_CHUNK; ++r) slot[r] = slot_of[L[r]];
    }
#pragma unroll
    for (int r = 0; r < MR_CHUNK; ++r) {
      const int y = yb + r;
      if (y >= y1 || !valid) continue;
      const int cur = slot[r];
      const u32 p = (u32)(x * h + y);
      if (cur != prev) {
#pragma unroll
        for (int side = 0; side < 2; ++side) {
          const int s = side ? cur : prev;
          if (s >= K) continue;                                          // (no slot: an unlisted id, or the virtual pixel before pixel 0)
          if (EMIT) {
            const u64 j = base[s] + a[s * 64 + lane];
            if (j < capacity) runs[j] = p - b[s * 64 + lane];
          }
          a[s * 64 + lane] += 1;
          b[s * 64 + lane] = p;
        }
      }
      if (!EMIT && cur < K) a[cur * 64 + lane] += 1u << 16;
      prev = cur;
    }
  }
  if (!EMIT && valid)
    for (int s = 0; s < K; ++s) cells[((size_t)s * w + x) * F.segs + g] = make_uint2(a[s * 64 + lane], b[s * 64 + lane]);
}

// (1) and (4): blockIdx.y = frame, the four waves of a workgroup are units 4 blockIdx.x .. + 3 of the frame, unit = segment * tiles_x + column
// tile.  The grid is sized for the launch's largest frame.
template <bool EMIT>
__global__ __launch_bounds__(256) void k_runs_walk(const long long* __restrict__ table, int n, long long stride, void* __restrict__ work,
                                                   const long long* __restrict__ heads, u32* __restrict__ runs, u64 capacity) {
  __shared__ u32 sa[4][OB_SLOTS * 64];
  __shared__ u32 sb[4][OB_SLOTS * 64];
  __shared__ u64 base[OB_SLOTS];
  __shared__ unsigned char slot_of[256];
  const int f = blockIdx.y;
  MrFrame F;
  if (f >= n || !mr_frame(table, f, stride, F)) return;                  // (uniform per workgroup, before the barrier)
  const int units = F.tiles_x * F.segs;
  if ((int)blockIdx.x * 4 >= units) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (!F.stack) {
    int s = OB_NONE;                                                     // id `tid` -> the FIRST slot that lists it
    for (int k = F.K - 1; k >= 0; --k) s = F.ids[k] == tid ? k : s;
    slot_of[tid] = (unsigned char)s;
  }
  if (tid < OB_SLOTS) base[tid] = (EMIT && tid < F.K) ? (u64)heads[((size_t)f * OB_SLOTS + tid) * MR_HEAD + RH_OFFSET] : 0;
  __syncthreads();
  const int u = blockIdx.x * 4 + wave;
  if (u >= units) return;
  uint2* cells = (uint2*)((u32*)work + (size_t)n * OB_SLOTS) + (size_t)f * (size_t)stride;
  mr_walk<EMIT>(F, slot_of, (u % F.tiles_x) * MR_TW, u / F.tiles_x, lane, sa[wave], sb[wave], cells, base, runs, capacity);
}

__device__ __forceinline__ u64 mr_shfl_up64(u64 v, int d) {
  const u32 lo = __shfl_up((u32)v, d, 64), hi = __shfl_up((u32)(v >> 32), d, 64);
  return ((u64)hi << 32) | lo;
}

// (2): blockIdx = (slot, frame).  The slot's w x segs cells, 1024 at a time: a cell's {boundaries | pixels << 16, last boundary} becomes {the
// boundaries of the cells before it, the last boundary before it}.  Then the head: { boundaries + 1, (offset: k_runs_heads), pixels, id }, and
// the slot's last boundary for the list's last element.  A slot >= K, or of a frame the device row refuses: four zeros.
__global__ __launch_bounds__(1024) void k_runs_scan(const long long* __restrict__ table, int n, long long stride, void* __restrict__ work,
                                                    long long* __restrict__ heads) {
  __shared__ u32 wc[16], wl[16], wa[16];
  const int s = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (f >= n) return;
  long long* hd = heads + ((size_t)f * OB_SLOTS + s) * MR_HEAD;
  u32* last = (u32*)work;
  MrFrame F;
  if (!mr_frame(table, f, stride, F) || s >= F.K) {                      // (uniform per workgroup)
    if (tid < MR_HEAD) hd[tid] = 0;
    if (tid == 0) last[(size_t)f * OB_SLOTS + s] = 0;
    return;
  }
  const int C = F.w * F.segs;                                            // (<= 2^22)
  uint2* cells = (uint2*)((u32*)work + (size_t)n * OB_SLOTS) + (size_t)f * (size_t)stride + (size_t)s * C;
  u32 carry_c = 0, carry_l = 0, area = 0;                                // (boundaries and pixels of a slot are <= h w <= 2^28)
  for (int i0 = 0; i0 < C; i0 += 1024) {
    const int i = i0 + tid;
    const uint2 v = i < C ? cells[i] : make_uint2(0u, 0u);
    const u32 c = v.x & 0xffffu;
    area += v.x >> 16;
    u32 ic = c, il = v.y;                                                // inclusive over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u32 tc = __shfl_up(ic, d, 64), tl = __shfl_up(il, d, 64);
      if (lane >= d) { ic += tc; il = max(il, tl); }
    }
    u32 el = __shfl_up(il, 1, 64);                                       // exclusive maximum
    if (lane == 0) el = 0;
    if (lane == 63) { wc[wave] = ic; wl[wave] = il; }
    __syncthreads();
    u32 pre_c = carry_c, pre_l = carry_l;
    for (int j = 0; j < 16; ++j) {
      const u32 cj = wc[j], lj = wl[j];
      if (j < wave) { pre_c += cj; pre_l = max(pre_l, lj); }
      carry_c += cj;
      carry_l = max(carry_l, lj);
    }
    if (i < C) cells[i] = make_uint2(pre_c + ic - c, max(pre_l, el));
    __syncthreads();                                                     // (the next round overwrites wc, wl)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) area += __shfl_xor(area, off, 64);
  if (lane == 0) wa[wave] = area;
  __syncthreads();
  if (tid == 0) {
    u32 tot = 0;
    for (int j = 0; j < 16; ++j) tot += wa[j];
    hd[RH_COUNT] = (long long)carry_c + 1;
    hd[RH_OFFSET] = 0;
    hd[RH_AREA] = tot;
    hd[RH_ID] = F.ids[s];
    last[(size_t)f * OB_SLOTS + s] = carry_l;
  }
}

// (3): one workgroup.  offset = the exclusive sum of the counts over (frame, slot) in order; a slot not in use keeps its zeros.  The last
// element of every list in use, N - its last boundary, when it is below the capacity.
__global__ __launch_bounds__(1024) void k_runs_heads(const long long* __restrict__ table, int n, const void* __restrict__ work,
                                                     long long* __restrict__ heads, u32* __restrict__ runs, u64 capacity) {
  __shared__ u64 wt[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const u32* last = (const u32*)work;
  const int E = n * OB_SLOTS;                                            // (<= 2^20)
  u64 carry = 0;
  for (int e0 = 0; e0 < E; e0 += 1024) {
    const int e = e0 + tid;
    const u64 c = e < E ? (u64)heads[(size_t)e * MR_HEAD + RH_COUNT] : 0;
    u64 ic = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const u64 t = mr_shfl_up64(ic, d);
      if (lane >= d) ic += t;
    }
    if (lane == 63) wt[wave] = ic;
    __syncthreads();
    u64 pre = carry;
    for (int j = 0; j < 16; ++j) {
      const u64 tj = wt[j];
      if (j < wave) pre += tj;
      carry += tj;
    }
    if (c > 0) {                                                         // (k_runs_scan found the frame's device row good)
      const u64 off = pre + ic - c;
      heads[(size_t)e * MR_HEAD + RH_OFFSET] = (long long)off;
      const long long* row = table + (size_t)OB_ROW * (e / OB_SLOTS);
      const u64 j = off + c - 1;
      if (j < capacity && ob_check(row) == OB_OK) runs[j] = (u32)(row[OW_H] * row[OW_W]) - last[e];
    }
    __syncthreads();
  }
}

static int mr_check_call(const char* who, const long long* table_host, int n, size_t run_capacity, long long* stride) {
  FRTM_CHECK_ARG(table_host, "%s: bad argument (a null table)", who);
  FRTM_CHECK_ARG(n >= 1 && n <= 65535, "%s: n = %d frames (1 .. 65535)", who, n);
  FRTM_CHECK_ARG(run_capacity >= 1 && (u64)run_capacity <= MR_MAXCAP, "%s: run_capacity = %zu elements (1 .. 2^40)", who, run_capacity);
  if (ob_check_table(who, table_host, n) != FRTM_OK) return FRTM_ERR_ARG;
  long long cells = 0;
  for (int i = 0; i < n; ++i) cells = max(cells, mr_cells(table_host + (size_t)OB_ROW * i));
  *stride = cells;
  return FRTM_OK;
}

extern "C" size_t frtm_encode_work_bytes(const long long* table_host, int n, size_t run_capacity) {
  long long stride = 0;
  if (mr_check_call("frtm_encode_work_bytes", table_host, n, run_capacity, &stride) != FRTM_OK) return 0;
  return mr_work_bytes(n, stride);
}

extern "C" int frtm_encode_frames(const long long* table_host, const long long* table_dev, int n, long long* heads, size_t head_words,
                                  unsigned int* runs, size_t run_capacity, void* work, size_t work_bytes, frtm_stream_t stream) {
  const char* who = "frtm_encode_frames";
  FRTM_CHECK_ARG(table_host && table_dev, "%s: bad argument (a null table)", who);
  FRTM_CHECK_ARG(heads && runs && work, "%s: bad argument (a null heads, runs or work)", who);
  FRTM_CHECK_ARG(!((uintptr_t)heads & 7) && !((uintptr_t)runs & 3) && !((uintptr_t)work & 7),
                 "%s: heads and work are 8-byte aligned and runs 4-byte aligned (got %p, %p, %p)", who, (void*)heads, work, (void*)runs);
  long long stride = 0;
  if (mr_check_call(who, table_host, n, run_capacity, &stride) != FRTM_OK) return FRTM_ERR_ARG;
  FRTM_CHECK_ARG(head_words >= (size_t)n * OB_SLOTS * MR_HEAD, "%s: heads holds %zu words, %d frames need %zu", who, head_words, n,
                 (size_t)n * OB_SLOTS * MR_HEAD);
  FRTM_CHECK_ARG(work_bytes >= mr_work_bytes(n, stride), "%s: work holds %zu bytes, frtm_encode_work_bytes asks for %zu", who, work_bytes,
                 mr_work_bytes(n, stride));
  int units = 0;                                                         // of the launch's largest frame (<= 256 * 256)
  for (int i = 0; i < n; ++i) {
    const long long* r = table_host + (size_t)OB_ROW * i;
    units = max(units, ceil_div((int)r[OW_W], MR_TW) * ceil_div((int)r[OW_H], MR_SEG));
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 gw(ceil_div(units, 4), n), gs(OB_SLOTS, n);
  k_runs_walk<false><<<gw, 256, 0, st>>>(table_dev, n, stride, work, heads, runs, (u64)run_capacity);
  FRTM_LAUNCH_CHECK();
  k_runs_scan<<<gs, 1024, 0, st>>>(table_dev, n, stride, work, heads);
  FRTM_LAUNCH_CHECK();
  k_runs_heads<<<1, 1024, 0, st>>>(table_dev, n, work, heads, runs, (u64)run_capacity);
  FRTM_LAUNCH_CHECK();
  k_runs_walk<true><<<gw, 256, 0, st>>>(table_dev, n, stride, work, heads, runs, (u64)run_capacity);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}
