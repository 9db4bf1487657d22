// What the two resident solver kernels share (k_cg_run_persistent in cg_persistent.hip, k_joint_run_persistent in joint_persistent.hip;
// included by these two files only): the exchange primitives and the grid barrier with its abort word, the fixed-order sums, the four
// compute phases over feature rows that stay in registers, and the host-side budget / time-out / reset of a launch.
//
// Everything on the device side is a force-inlined template: k_cg_run_persistent needs 254 of the 256 VGPRs a 512-thread workgroup may
// have, and a grid that must be co-resident cannot afford a call's register pressure (tests/test_isa_invariants.py pins the budget).
// The sums below are not associative: the order of operations in the phases is part of the result and must not be rearranged.
#pragma once
#include "frtm_common.h"
#include "../../include/frtm_hip.h"

namespace resident {

constexpr int NT = 512;            // threads per workgroup (8 waves: one workgroup per CU, up to 256 VGPRs per lane)
constexpr int NWAVE = 8;
constexpr int CPW = 12;            // channels per wave: a workgroup holds 96 channels
constexpr int PW = 66;             // LDS row pitch of s / t (x = -1 .. 64)
constexpr int FN = CPW * NWAVE * 9;        // 864: a 3x3 filter over the workgroup's channels = one weight-gradient slab
// per kernel: RMAX output rows per workgroup; RMAX + 4 feature rows per lane (xr), RMAX + 2 score rows (stencil halo)

// Memory model of the exchange (guide: "inter-workgroup communication", form R1): payloads are sc1 / write-through stores, EVERY storing
// wave drains them with s_waitcnt vmcnt(0) before the workgroup's arrival is counted, consumers read them with sc1 loads (L1-bypassing),
// so neither an L2 write-back nor an L1 invalidate is needed.
__device__ __forceinline__ void st_wt(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_l2(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The launch's abort word has three states, every transition a compare-and-swap from 0:
//   0 running   1 ABORTED (a workgroup gave up waiting; counted once in stats[2]; nobody writes anything back)
//   2 COMMITTED (workgroup 0 claimed it behind the last barrier: every workgroup has arrived there; stats[3] counts the committed launches,
//     so the host can tell how many Gauss-Newton iterations of a run() really happened and re-runs only the missed ones)
// COMMIT XOR ABORT: a workgroup whose spin runs out in the very barrier the others have just passed either wins the word (-> 1: nobody
// writes, workgroup 0's claim fails) or finds it committed (-> it has been waited for, the barrier is complete: it passes like everybody
// else).  A launch is never both counted as aborted and partially written.  Waiters leave a barrier on 1 only.
// Every polled word (arrivals, abort word) is zeroed by a memset node in front of EVERY launch (resident_reset_words; also under graph
// replay): a launch never inherits state from the one before it.  Every spin is bounded: on a time-out (another resident-hungry kernel
// holds the CUs) the launch aborts without writing its results, bumps the sticky abort counter stats[2] and the host re-runs the solve
// in the multi-kernel form (model/optimizer.py).
// k_cg_run_persistent used exchanges before (give up: exchange(1), counted if the old value was 0; leave on != 0; commit: exchange(2),
// won if the old value was 0).  The two forms leave w2, vec, state and stats[0..3] the same: (a) time-out before the claim: the
// exchange returned 0 / the CAS 0 -> 1 wins, the abort is counted once, workgroup 0's later claim finds 1 and writes nothing;
// (b) time-out after the claim (only in the last barrier, which is then complete): the exchange returned 2 / the CAS fails with 2,
// nothing is counted; the waiter used to leave and now passes, repeats the redundant vector step and exits -- it is not workgroup 0
// and writes nothing either way (the old exchange left the word at 1 then, the CAS leaves it at 2: nobody reads it afterwards);
// (c) leaving on != 0 against == 1 differs for the value 2 only, which is case (b).
__device__ __forceinline__ bool give_up_or_committed(unsigned* abort_flag, unsigned* stats) {
  unsigned expected = 0u;
  const bool won = __hip_atomic_compare_exchange_strong(abort_flag, &expected, 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (won && stats) __hip_atomic_fetch_add(stats + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return !won && expected == 2u;        // true: committed meanwhile (only possible in the last barrier, which is then complete)
}
// Workgroup 0's claim behind the last barrier, BEFORE anything is written: 0 -> 2.  Returns the word's state afterwards: 2 committed
// (counted in stats[3]), 1 somebody gave up first (the abort is already counted and NOTHING may be written).
__device__ __forceinline__ unsigned claim_commit(unsigned* abort_flag, unsigned* stats) {
  unsigned expected = 0u;
  const bool won = __hip_atomic_compare_exchange_strong(abort_flag, &expected, 2u, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (won && stats) __hip_atomic_fetch_add(stats + 3, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return won ? 2u : expected;
}

// Grid barrier on a monotonic counter (target = epoch * workgroups).  Returns false (in every thread of the workgroup) if the launch was aborted.
__device__ __forceinline__ bool grid_sync(unsigned* counter, unsigned* abort_flag, unsigned* stats, unsigned target, long long limit, int* sh_flag) {
  // EVERY wave drains its own write-through stores of the phase before the workgroup is counted as arrived: the barrier below only
  // orders waves inside the CU, it does not wait for another wave's stores to leave it (guide pitfall 14).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const long long t0 = wall_clock64();
    int ok = 1;
    while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
      __builtin_amdgcn_s_sleep(2);
      if (__hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1u) { ok = 0; break; }
      // default 4 ms at 100 MHz: some workgroup never became resident
      if (wall_clock64() - t0 > limit) { ok = give_up_or_committed(abort_flag, stats) ? 1 : 0; break; }
    }
    *sh_flag = ok;
  }
  __syncthreads();
  return *sh_flag != 0;
}

// XCD-hierarchical form of the barrier (guide: "barrier-xcd").  A flat barrier serialises 240 agent-scope atomics on ONE address and
// has 240 pollers on it; here the workgroups of an XCD (30 of them) arrive on their XCD's counter, the LAST arriver of each XCD
// arrives on the top counter and polls it (8 arrivals, 8 pollers), then publishes the epoch in its XCD's generation word, which the
// other workgroups of that XCD poll.  Which XCD a workgroup runs on is read from the hardware (HW_REG_XCC_ID), never assumed: the
// per-XCD populations are counted at kernel start, behind the first (flat) barrier (GridBarrier::join).  hbar layout (unsigned words,
// 16-word = 64-byte pitch so that no two polled words share a line): [16 x] arrivals, [128 + 16 x] generation, [256] top, [272 + x] population.
constexpr int HB_ARR = 0, HB_GEN = 128, HB_TOP = 256, HB_POP = 272, HB_WORDS = 288;
static_assert(HB_WORDS == FRTM_HBAR_WORDS, "the callers allocate FRTM_HBAR_WORDS words of hbar");
__device__ __forceinline__ bool hier_sync(unsigned* hbar, unsigned* abort_flag, unsigned* stats, int xcc, unsigned n_x, unsigned n_active,
                                          unsigned epoch, long long limit, int* sh_flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every wave: its write-through stores of the phase have left the CU
  __syncthreads();
  if (threadIdx.x == 0) {
    int ok = 1;
    const long long t0 = wall_clock64();
    const unsigned old = __hip_atomic_fetch_add(hbar + HB_ARR + 16 * xcc, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old + 1u == epoch * n_x) {                      // last arriver of this XCD: speaks for it at the top level
      __hip_atomic_fetch_add(hbar + HB_TOP, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      while (__hip_atomic_load(hbar + HB_TOP, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < epoch * n_active) {
        __builtin_amdgcn_s_sleep(1);
        if (__hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1u) { ok = 0; break; }
        if (wall_clock64() - t0 > limit) { ok = give_up_or_committed(abort_flag, stats) ? 1 : 0; break; }
      }
      if (ok) __hip_atomic_store(hbar + HB_GEN + 16 * xcc, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      while (__hip_atomic_load(hbar + HB_GEN + 16 * xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < epoch) {
        __builtin_amdgcn_s_sleep(1);
        if (__hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1u) { ok = 0; break; }
        if (wall_clock64() - t0 > limit) { ok = give_up_or_committed(abort_flag, stats) ? 1 : 0; break; }
      }
    }
    *sh_flag = ok;
  }
  __syncthreads();
  return *sh_flag != 0;
}

// A kernel's barrier state.  bar[0] arrivals of the flat barrier, bar[2] abort word of THIS launch; hbar == nullptr: every barrier is
// the flat one.  sh: 4 ints of LDS (the barrier's verdict; XCD id, workgroups on this XCD, populated XCDs).
struct GridBarrier {
  unsigned* bar; unsigned* hbar; unsigned* stats; long long limit; int* sh;
  int xcc = 0; unsigned n_x = 1, n_active = 1, epoch = 0, hepoch = 0;

  __device__ __forceinline__ GridBarrier(unsigned* bar_, unsigned* hbar_, unsigned* stats_, long long limit_, int* sh_)
      : bar(bar_), hbar(hbar_), stats(stats_), limit(limit_), sh(sh_) {}
  __device__ __forceinline__ unsigned* abort_flag() const { return bar + 2; }
  __device__ __forceinline__ bool flat_sync() { return grid_sync(bar, abort_flag(), stats, (++epoch) * gridDim.x, limit, sh); }
  // Which XCD am I on, and how many workgroups does each XCD hold?  Registration, then ONE flat barrier.  False: the launch was aborted.
  __device__ __forceinline__ bool join() {
    if (threadIdx.x == 0) sh[0] = 1;
    if (hbar != nullptr) {
      if (threadIdx.x == 0) {
        const int x = (int)(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u);          // HW_REG_XCC_ID, bits [3:0]
        sh[1] = x;
        __hip_atomic_fetch_add(hbar + HB_POP + x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
      if (!flat_sync()) return false;
      if (threadIdx.x == 0) {
        unsigned act = 0, mine = 0;
        for (int x = 0; x < 8; ++x) {
          const unsigned c_ = __hip_atomic_load(hbar + HB_POP + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          act += c_ > 0u ? 1u : 0u;
          if (x == sh[1]) mine = c_;
        }
        sh[2] = (int)mine; sh[3] = (int)act;
      }
      __syncthreads();
      xcc = sh[1]; n_x = (unsigned)sh[2]; n_active = (unsigned)sh[3];
    }
    __syncthreads();
    return true;
  }
  __device__ __forceinline__ bool sync() {
    if (hbar != nullptr) return hier_sync(hbar, abort_flag(), stats, xcc, n_x, n_active, ++hepoch, limit, sh);
    return flat_sync();
  }
};

// 64-lane sum that lands in lane 63 only: six DPP adds on the VALU (prefix within the 16-lane rows, then row broadcasts) -- no
// LDS crossbar traffic, unlike a __shfl_xor butterfly (ds_bpermute / ds_swizzle per step).  Fixed order.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
  const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true);     // bound_ctrl: lanes without a source read 0
  return v + __int_as_float(moved);
}
__device__ __forceinline__ float wave_sum_to63(float v) {
  v = dpp_add<0x111, 0xf>(v);      // row_shr:1
  v = dpp_add<0x112, 0xf>(v);      // row_shr:2
  v = dpp_add<0x114, 0xf>(v);      // row_shr:4
  v = dpp_add<0x118, 0xf>(v);      // row_shr:8   -> lane 15 of every row holds the row total
  v = dpp_add<0x142, 0xa>(v);      // row_bcast:15 into rows 1 and 3
  v = dpp_add<0x143, 0xc>(v);      // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave total
  return v;
}

// deterministic block sums of two values over NW waves (fixed butterfly + fixed wave order); all threads receive the totals; red: 32 floats
template <int NW = NWAVE>
__device__ __forceinline__ void bsum2(float& a, float& b, float* red) {
  a = wave_sum_to63(a);
  b = wave_sum_to63(b);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 63) { red[wid] = a; red[16 + wid] = b; }
  __syncthreads();
  float ta = 0.f, tb = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) { ta += red[i]; tb += red[16 + i]; }
  a = ta; b = tb;
}

// ---- the phases over the resident rows: workgroup = 8 waves x 12 channels, lane = x, rows [r0, r0 + R) of one sample, R <= PR <= RMAX ----

// Feature rows [r0 - 2, r0 + PR + 2) of this wave's channels into registers; the workgroup's channels are the maps first .. first + cnt - 1
// of X (zeros beyond them, beyond the map and beyond the PR + 4 rows a workgroup of this launch holds).
// The scalars come BY REFERENCE on purpose: by value the compiler simplifies this function on its own before it inlines it, folds the
// 168 load conditions into per-row lane masks that stay live in SGPR pairs, and k_cg_run_persistent ends up with 255 VGPRs and SGPR spills.
template <int RMAX>
__device__ __forceinline__ void load_rows(float (&xr)[CPW][RMAX + 4], const float* X, size_t first, const int& cnt, const int& h, const int& w,
                                          const int& r0, const int& PR, const int& lane, const int& wid) {
  const int hw = h * w;
#pragma unroll
  for (int k = 0; k < CPW; ++k) {
    const int ch = wid * CPW + k;
    const float* Xc = X + (first + min(ch, cnt - 1)) * hw;
#pragma unroll
    for (int i = 0; i < RMAX + 4; ++i) {
      const int yy = r0 - 2 + i;
      const bool ok = ch < cnt && lane < w && (unsigned)yy < (unsigned)h && i < PR + 4;
      xr[k][i] = ok ? Xc[yy * w + lane] : 0.f;
    }
  }
}

// The workgroup's rows of B (9 taps) and c of sample n_s into LDS for the whole launch; s and t start as zeros (their borders stay zero).
template <int RMAX>
__device__ __forceinline__ void load_maps(float (*Bl)[RMAX][64], float (*cl)[64], float (*sl)[PW], float (*tl)[PW], const float* Bm, const float* cm,
                                          int n_s, int h, int w, int r0, int R) {
  const int tid = threadIdx.x, hw = h * w;
  for (int i = tid; i < 9 * RMAX * 64; i += NT) {
    const int d = i / (RMAX * 64), rr = (i / 64) % RMAX, x = i & 63;
    (&Bl[0][0][0])[i] = (rr < R && x < w) ? Bm[((size_t)n_s * 9 + d) * hw + (r0 + rr) * w + x] : 0.f;
  }
  for (int i = tid; i < RMAX * 64; i += NT) {
    const int rr = i / 64, x = i & 63;
    (&cl[0][0])[i] = (rr < R && x < w) ? cm[(size_t)n_s * hw + (r0 + rr) * w + x] : 0.f;
  }
  for (int i = tid; i < (RMAX + 2) * PW; i += NT) (&sl[0][0])[i] = 0.f;
  for (int i = tid; i < RMAX * PW; i += NT) (&tl[0][0])[i] = 0.f;
}

// Scores of the workgroup's channels under the 3x3 filter f (LDS, [96][9], zero beyond the channels that exist) for the rows
// [r0 - 1, r0 + R]: per lane three column-partial sums (no shuffles in the channel loop), x +- 1 by two lane shifts, the 8 channel
// groups combined through LDS in a fixed order; element i = row * 64 + x of the combined rows goes to sink(i, sum).
template <int RMAX, class Sink>
__device__ __forceinline__ void partial_scores(const float (&xr)[CPW][RMAX + 4], const float* f_all, float (*red)[RMAX + 2][64], Sink sink) {
  constexpr int SR = RMAX + 2;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float S0[SR], S1[SR], S2[SR];
#pragma unroll
  for (int j = 0; j < SR; ++j) { S0[j] = 0.f; S1[j] = 0.f; S2[j] = 0.f; }
#pragma unroll
  for (int k = 0; k < CPW; ++k) {
    const float* f = f_all + (wid * CPW + k) * 9;          // LDS broadcast reads
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const float f0 = f[dy * 3 + 0], f1 = f[dy * 3 + 1], f2_ = f[dy * 3 + 2];
#pragma unroll
      for (int j = 0; j < SR; ++j) {
        const float xv = xr[k][j + dy];
        S0[j] += f0 * xv; S1[j] += f1 * xv; S2[j] += f2_ * xv;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < SR; ++j) {
    // tap dx = 0 reads the pixel to the LEFT (x - 1), dx = 2 the one to the right; lanes >= w hold zeros
    const float l = __shfl_up(S0[j], 1, 64), r = __shfl_down(S2[j], 1, 64);
    red[wid][j][lane] = (lane > 0 ? l : 0.f) + S1[j] + (lane < 63 ? r : 0.f);
  }
  __syncthreads();
  for (int i = tid; i < SR * 64; i += NT) {
    const int j = i >> 6, x = i & 63;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < NWAVE; q += 4) s += (red[q][j][x] + red[q + 1][j][x]) + (red[q + 2][j][x] + red[q + 3][j][x]);
    sink(i, s);
  }
}

// t = sw (B s - c?) on the workgroup's rows (wave = rows wid, wid + 8); s holds the full scores with their halo.  Ends behind a barrier.
template <int RMAX>
__device__ __forceinline__ void stencil(float (*Bl)[RMAX][64], float (*cl)[64], float (*sl)[PW], float (*tl)[PW], int R, int w, bool with_c, float swn) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int rr = wid; rr < RMAX; rr += NWAVE) {
    float acc = 0.f;
    if (rr < R && lane < w) {
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) acc += Bl[dy * 3 + dx][rr][lane] * sl[rr + dy][lane + dx];
      if (with_c) acc -= cl[rr][lane];
      acc *= swn;
    }
    tl[rr][lane + 1] = acc;
  }
  __syncthreads();
}

// Weight gradient g[ch, dy, dx] = sum_u t[u] X[ch, u + (dy - 1, dx - 1)] of the workgroup's channels from the SAME registers, t taken
// shifted from LDS, 64-lane sums -> staged in gl (LDS, FN floats) -> the workgroup's slab in global memory (write-through stores).
template <int RMAX>
__device__ __forceinline__ void weight_gradient(const float (&xr)[CPW][RMAX + 4], float (*tl)[PW], float* gl, float* slab) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  float tv[RMAX][3];
#pragma unroll
  for (int rr = 0; rr < RMAX; ++rr)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) tv[rr][dx] = tl[rr][lane + 2 - dx];
#pragma unroll
  for (int k = 0; k < CPW; ++k) {
    float a[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) a[e] = 0.f;
#pragma unroll
    for (int rr = 0; rr < RMAX; ++rr)
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        const float xv = xr[k][rr + dy + 1];
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) a[dy * 3 + dx] += tv[rr][dx] * xv;
      }
    float* dst = gl + (wid * CPW + k) * 9;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const float tot = wave_sum_to63(a[e]);
      if (lane == 63) dst[e] = tot;
    }
  }
  __syncthreads();
  for (int i = tid; i < FN; i += NT) st_wt(slab + i, gl[i]);
}

// ---- host side ----

// Workgroups a resident launch may use: one 512-thread workgroup per CU (256 VGPRs per lane, ~80 KB of LDS or more), on at most 15/16 of
// the CUs of THIS device (240 of an MI355X's 256: the rest stays free for kernels of other streams; a partitioned or CU-masked device
// gets a proportionally smaller budget and takes the multi-kernel form sooner).  Cached per device.
static inline int resident_budget() {
  static int cached[16] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return 240; }
  if (cached[dev] == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
    cached[dev] = cus - cus / 16;
  }
  return cached[dev];
}

// Barrier time-out in 10 ns ticks (4 ms).  debug_abort: the first workgroup to wait gives up at once -- tests of the callers' fallback.
static inline long long resident_spin_limit(int debug_abort) { return debug_abort ? 0LL : 400000LL; }

// Every polled word starts at zero in EVERY launch (memset nodes: also when the launch is replayed from a hipGraph); bar[3] is the
// phase-stamp switch of tools/cg_phase_times.py and is left alone.
static inline int resident_reset_words(unsigned* bar, unsigned* hbar, hipStream_t stream) {
  FRTM_HIP(hipMemsetAsync(bar, 0, 3 * sizeof(unsigned), stream));
  if (hbar) FRTM_HIP(hipMemsetAsync(hbar, 0, HB_WORDS * sizeof(unsigned), stream));
  return FRTM_OK;
}

}  // namespace resident
