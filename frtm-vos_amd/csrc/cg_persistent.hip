// One Gauss-Newton iteration of the FILTER problem (reference optimizer.py:77-153 on discriminator.py:187-196: right-hand side,
// `iters` conjugate-gradient steps, x += step * delta) as ONE persistent launch for gfx950.
//
// The multi-kernel form (scores -> stencil -> weight gradient -> CG step) spends 53 us per CG iteration for 25 us of kernel
// time: four dependent launches per iteration.  Here the memory's feature maps X (N x c x h x w, 49.8 MB at N = 80, 480p) are
// read from HBM ONCE per run and stay in VECTOR REGISTERS for all iters + 1 operator applications:
//
//   workgroup (n, part) owns the rows [r0, r0 + R) of sample n: 8 waves, wave = channel group (c / 8 channels), lane = x.
//   Each lane keeps X[n, ch, r0-2 .. r0+R+1, x] for its wave's channels (12 x 14 floats at c = 96, R = 10), i.e. the rows the
//   score halo (for the stencil) and the weight gradient need.  Per operator application, inside the workgroup:
//     scores   s = X * v      per lane three column-partial sums (no shuffles in the channel loop), x +- 1 by two lane shifts,
//                             channel groups combined through LDS in a fixed order
//     stencil  t = sw (B s - c)   B, c rows of this workgroup live in LDS for the whole run
//     wgrad    g[c,dy,dx] = sum_u t[u] X[c, u + (dy-1, dx-1)]   from the SAME registers, t taken shifted from LDS,
//                             64-lane butterfly sums -> one 864-float slab per workgroup (write-through stores)
//   then across workgroups: grid barrier, every workgroup sums a few elements over all slabs (fixed order), grid barrier, every
//   workgroup reads the 864 sums and performs the CG vector step REDUNDANTLY in its own LDS copy of (b, r, r_prev, p, x): the
//   same instructions on the same inputs give bit-identical vectors everywhere, so no third exchange is needed.
// Two grid barriers per application (monotonic counter, agent-scope atomics).  The barrier, its abort word (commit XOR abort), the memory model
// of the exchange, the fixed-order sums and the phases over the resident rows are shared with the joint problem's kernel: resident_grid.h.
// A launch that times out aborts without touching x; the host re-runs the solve in the multi-kernel form (model/optimizer.py).
// All sums have a fixed order: results are deterministic.
#include "resident_grid.h"

namespace {

using namespace resident;          // NT, NWAVE, CPW, PW; the barrier, the sums and the phases
constexpr int RMAX = 10;           // output rows per workgroup
constexpr int XR = RMAX + 4;       // X rows held per lane
constexpr int SR = RMAX + 2;       // score rows (stencil halo)
constexpr int NMAX = FN;           // 864

struct Params {
  const float* X; const float* Bm; const float* cm; const float* sw;
  float* w2; float* vec; float* state; float* slabs; float* qbuf; unsigned* bar; unsigned* hbar;
  int N, c, h, w, R, parts, iters, has_p, apply_dff, fr, std_alpha, parity;
  float dff, lam2, invM, step;
  const int* guard; int guard_min; unsigned* stats;     // optional device-side early-out and its counters (see the guarded entry)
  int count_run;                                        // add this launch to stats[0] (completed) / stats[1] (skipped by the guard)
  long long spin_limit;                                 // barrier time-out in 10 ns ticks
};

// LDS carve-up (floats); ~80 KB, so the kernel takes its LDS dynamically (more than the 64 KB a static allocation may have)
constexpr int L_VEC = 0;                              // 7 vectors of NMAX: b, r, r_prev, p, q (also the slab staging), x, w
constexpr int L_B = L_VEC + 7 * NMAX;                 // [9][RMAX][64]
constexpr int L_C = L_B + 9 * RMAX * 64;              // [RMAX][64]
constexpr int L_S = L_C + RMAX * 64;                  // [SR][PW]
constexpr int L_T = L_S + SR * PW;                    // [RMAX][PW]
constexpr int L_RED = L_T + RMAX * PW;                // [NWAVE][SR][64]
constexpr int L_SRED = L_RED + NWAVE * SR * 64;       // 32
constexpr int L_FLAG = L_SRED + 32;                   // 1 int (+ 3 ints: xcc id, workgroups on this XCD, populated XCDs)
constexpr int L_TOTAL = L_FLAG + 4;

__global__ __launch_bounds__(NT) void k_cg_run_persistent(const Params P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* vb = lds + L_VEC; float* vr = vb + NMAX; float* vrp = vr + NMAX; float* vp = vrp + NMAX; float* vq = vp + NMAX;
  float* vx = vq + NMAX; float* vw = vx + NMAX;
  float (*Bl)[RMAX][64] = (float (*)[RMAX][64])(lds + L_B);
  float (*cl)[64] = (float (*)[64])(lds + L_C);
  float (*sl)[PW] = (float (*)[PW])(lds + L_S);
  float (*tl)[PW] = (float (*)[PW])(lds + L_T);
  float (*red)[SR][64] = (float (*)[SR][64])(lds + L_RED);
  float* gl = vq;                                     // slab staging: consumed (stored) before vq is written
  float* sred = lds + L_SRED;
  int* sh_flag_p = (int*)(lds + L_FLAG);

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int G = gridDim.x, g = blockIdx.x;
  // Device-side form of the reference's early-out (discriminator.py:214: fewer than 10 mask pixels above 0.5 -> no update): the count
  // was left in device memory by an earlier kernel of this stream, every workgroup reads the same value and the whole launch
  // returns before its first barrier.  The host never has to wait for the count.
  if (P.guard != nullptr && *P.guard < P.guard_min) {
    if (g == 0 && tid == 0 && P.stats && P.count_run) atomicAdd(P.stats + 1, 1u);
    return;
  }
  const int n_s = g / P.parts, part = g - n_s * P.parts;
  const int r0 = part * P.R;
  const int R = min(P.R, P.h - r0);                   // rows this workgroup owns (>= 1 by construction)
  const int c = P.c, h = P.h, w = P.w, n = c * 9;
  GridBarrier gb(P.bar, P.hbar, P.stats, P.spin_limit, sh_flag_p);
  // optional phase stamps of workgroup 0 (bar[3] != 0): 10 ns ticks into qbuf[NMAX ..] as raw ints (tools/cg_phase_times.py)
  const bool stamp_on = (g == 0) && (P.bar[3] != 0u);
  int n_stamp = 0;
  auto stamp = [&]() { if (stamp_on && tid == 0 && n_stamp < 250) { ((int*)P.qbuf)[NMAX + n_stamp] = (int)(wall_clock64() & 0x7fffffff); } ++n_stamp; };
  stamp();

  // ---- resident data: X rows in registers, B / c rows and the vectors in LDS ----
  float xr[CPW][XR];
  load_rows<RMAX>(xr, P.X, (size_t)n_s * c, c, h, w, r0, P.R, lane, wid);
  load_maps<RMAX>(Bl, cl, sl, tl, P.Bm, P.cm, n_s, h, w, r0, R);
  for (int i = tid; i < NMAX; i += NT) {
    const bool on = i < n;
    vw[i] = on ? P.w2[i] : 0.f;
    vp[i] = (on && P.has_p) ? P.vec[3 * n + i] : 0.f;
    vrp[i] = (on && P.has_p) ? P.vec[2 * n + i] : 0.f;
    vb[i] = vr[i] = vq[i] = vx[i] = 0.f;
  }
  const float swn = P.sw[n_s];
  if (!gb.join()) return;                             // XCD registration behind ONE flat barrier; ends in a workgroup barrier (LDS above is set up)
  stamp();

  // ---- one operator application: vq <- sum_samples J^T (sw (B (X * v) - c?)) + lam2 v ----
  auto apply = [&](const float* v, bool with_c) -> bool {
    partial_scores<RMAX>(xr, v, red, [&](int i, float s) {          // (v: zero beyond n)
      const int j = i >> 6, x = i & 63;
      const int yy = r0 - 1 + j;
      sl[j][x + 1] = (x < w && (unsigned)yy < (unsigned)h && j < R + 2) ? s : 0.f;
    });
    __syncthreads();
    stamp();
    stencil<RMAX>(Bl, cl, sl, tl, R, w, with_c, swn);
    stamp();
    weight_gradient<RMAX>(xr, tl, gl, P.slabs + (size_t)g * NMAX);
    stamp();
    if (!gb.sync()) return false;
    stamp();
    // distributed fixed-order sum: workgroup g owns the elements [g * epw, (g + 1) * epw), one wave per element
    const int epw = (n + G - 1) / G;
    for (int e0 = wid; e0 < epw; e0 += NWAVE) {
      const int e = g * epw + e0;
      if (e < n) {
        float s = 0.f;
        for (int k = lane; k < G; k += 64) s += ld_l2(P.slabs + (size_t)k * NMAX + e);
        s = wave_sum_to63(s);
        if (lane == 63) st_wt(P.qbuf + e, s);
      }
    }
    stamp();
    if (!gb.sync()) return false;
    stamp();
    for (int i = tid; i < NMAX; i += NT) vq[i] = i < n ? ld_l2(P.qbuf + i) + P.lam2 * v[i] : 0.f;        // (gl aliases vq: its stores are long done)
    __syncthreads();
    stamp();
    return true;
  };

  // ---- right-hand side b = -(J^T f(w) + lam2 w)   (optimizer.py:80-85) ----
  if (!apply(vw, true)) return;
  // r = b; z = M^-1 r; rho' = <r,z>; rho2 = <r_prev,z>; first direction   (optimizer.py:107-130; k_cg_begin + k_cg_direction)
  float rho_cur;
  {
    float d0 = 0.f, d1 = 0.f;
    for (int i = tid; i < NMAX; i += NT) {
      const float bv = -vq[i];
      vb[i] = bv; vr[i] = bv;
      const float z = bv * P.invM;
      d0 += bv * z;
      if (P.has_p && !P.fr) d1 += vrp[i] * z;
    }
    bsum2(d0, d1, sred);
    float beta = 0.f;
    if (P.has_p) {
      float rho1 = P.state[0];
      if (P.apply_dff) rho1 = rho1 / P.dff;
      const float vv = P.fr ? d0 / rho1 : (d0 - d1) / rho1;
      beta = (vv < 0.f) ? 0.f : vv;
    }
    for (int i = tid; i < NMAX; i += NT) {
      const float z = vr[i] * P.invM;
      vp[i] = P.has_p ? (z + vp[i] * beta) : z;
    }
    rho_cur = d0;
    __syncthreads();
  }
  float alpha = 0.f, beta_last = 0.f, rho_prev = P.state[0];
  for (int it = 0; it < P.iters; ++it) {
    if (!apply(vp, false)) return;
    const bool first = it == 0, last = it == P.iters - 1;
    float pq = 0.f, pr = 0.f;
    for (int i = tid; i < NMAX; i += NT) { pq += vp[i] * vq[i]; pr += vp[i] * vr[i]; }
    bsum2(pq, pr, sred);
    alpha = P.std_alpha ? rho_cur / pq : pr / pq;
    float rn_ = 0.f, r2_ = 0.f;
    for (int i = tid; i < NMAX; i += NT) {
      const float rv = vr[i], pv = vp[i];
      vrp[i] = rv;
      vx[i] = first ? pv * alpha : vx[i] + pv * alpha;
      float rn = rv;
      if (!last) { rn = rv - vq[i] * alpha; vr[i] = rn; }
      const float z = rn * P.invM;
      rn_ += rn * z;
      r2_ += rv * z;
    }
    bsum2(rn_, r2_, sred);
    rho_prev = rho_cur;
    if (!last) {
      const float vv = P.fr ? rn_ / rho_cur : (rn_ - r2_) / rho_cur;
      beta_last = (vv < 0.f) ? 0.f : vv;
      for (int i = tid; i < NMAX; i += NT) vp[i] = vr[i] * P.invM + vp[i] * beta_last;
      rho_cur = rn_;
    }
    __syncthreads();
  }
  // ---- write back (one workgroup): x += step * delta and the carried solver state ----
  // Workgroup 0 claims the launch's abort word BEFORE it writes (commit XOR abort, resident_grid.h): if somebody gave up first, the
  // abort is already counted and NOTHING is written.
  if (g == 0) {
    if (tid == 0) sh_flag_p[0] = claim_commit(gb.abort_flag(), P.stats) == 2u ? 1 : 0;
    __syncthreads();
    if (!sh_flag_p[0]) return;
    for (int i = tid; i < n; i += NT) {
      P.w2[i] = vw[i] + P.step * vx[i];
      P.vec[0 * n + i] = vb[i];
      P.vec[1 * n + i] = vr[i];
      P.vec[2 * n + i] = vrp[i];
      P.vec[3 * n + i] = vp[i];
      P.vec[4 * n + i] = vq[i];
      P.vec[5 * n + i] = vx[i];
    }
    if (tid == 0) {
      // the multi-kernel form leaves: state[0] = rho of the last iteration, [4] = rho' of the next direction (if any), [1] alpha, [2] beta
      P.state[0] = P.iters > 0 ? rho_prev : P.state[0];
      P.state[4] = rho_cur;
      P.state[1] = alpha;
      P.state[2] = beta_last;
      if (P.stats && P.count_run) atomicAdd(P.stats, 1u);
    }
  }
}

}  // namespace

extern "C" {

int frtm_cg_persistent_plan(int N, int c, int h, int w, int* parts_out, int* rows_out) {
  if (N < 1 || c < 1 || c > CPW * NWAVE || w < 1 || w > 64 || h < 1) return 0;
  const int budget = resident_budget();
  const int min_parts = ceil_div(h, RMAX);
  if ((long)N * min_parts > budget) return 0;
  int parts = budget / N;
  if (parts > h) parts = h;
  if (parts < min_parts) parts = min_parts;
  int R = ceil_div(h, parts);
  parts = ceil_div(h, R);                       // no empty workgroups
  if (parts_out) *parts_out = parts;
  if (rows_out) *rows_out = R;
  return N * parts;
}

int frtm_cg_run_persistent_guarded(const float* X, const float* Bm, const float* cm, const float* sw, int N, int c, int h, int w,
                                   float* w2, float* vec, float* state, float* slabs, float* qbuf, unsigned* bar,
                                   int iters, int has_p, int apply_dff, int fletcher_reeves, int standard_alpha, float dff,
                                   float lam2, float invM, float step, const int* guard_count, int guard_min, unsigned* stats,
                                   int count_run, int debug_abort, unsigned* hbar, frtm_stream_t stream) {
  FRTM_CHECK_ARG(X && Bm && cm && sw && w2 && vec && state && slabs && qbuf && bar && iters >= 0, "frtm_cg_run_persistent: bad argument");
  int parts = 0, R = 0;
  const int G = frtm_cg_persistent_plan(N, c, h, w, &parts, &R);
  FRTM_CHECK_ARG(G > 0, "frtm_cg_run_persistent: problem (N=%d, c=%d, %dx%d) does not fit the resident form", N, c, h, w);
  Params P;
  P.X = X; P.Bm = Bm; P.cm = cm; P.sw = sw; P.w2 = w2; P.vec = vec; P.state = state; P.slabs = slabs; P.qbuf = qbuf; P.bar = bar;
  P.N = N; P.c = c; P.h = h; P.w = w; P.R = R; P.parts = parts; P.iters = iters; P.has_p = has_p; P.apply_dff = apply_dff;
  P.fr = fletcher_reeves; P.std_alpha = standard_alpha; P.parity = 0; P.dff = dff; P.lam2 = lam2; P.invM = invM; P.step = step;
  P.guard = guard_count; P.guard_min = guard_min; P.stats = stats; P.count_run = count_run; P.hbar = hbar;
  P.spin_limit = resident_spin_limit(debug_abort);
  static bool attr_set = false;
  if (!attr_set) {
    FRTM_HIP(hipFuncSetAttribute((const void*)k_cg_run_persistent, hipFuncAttributeMaxDynamicSharedMemorySize, L_TOTAL * 4));
    attr_set = true;
  }
  if (int e = resident_reset_words(bar, hbar, (hipStream_t)stream)) return e;
  k_cg_run_persistent<<<G, NT, L_TOTAL * 4, (hipStream_t)stream>>>(P);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

int frtm_cg_run_persistent(const float* X, const float* Bm, const float* cm, const float* sw, int N, int c, int h, int w,
                           float* w2, float* vec, float* state, float* slabs, float* qbuf, unsigned* bar,
                           int iters, int has_p, int apply_dff, int fletcher_reeves, int standard_alpha, float dff,
                           float lam2, float invM, float step, frtm_stream_t stream) {
  return frtm_cg_run_persistent_guarded(X, Bm, cm, sw, N, c, h, w, w2, vec, state, slabs, qbuf, bar, iters, has_p, apply_dff, fletcher_reeves,
                                        standard_alpha, dff, lam2, invM, step, nullptr, 0, nullptr, 0, 0, nullptr, stream);
}

}  // extern "C"
