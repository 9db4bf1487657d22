// One Gauss-Newton iteration of the JOINT first-frame problem (reference discriminator.py:154-199 on optimizer.py:77-153: variables
// project.weight (c, Cin, 1, 1) and filter.weight (1, c, 3, 3); right-hand side, `iters` conjugate-gradient steps, x += step * delta)
// as ONE persistent launch for gfx950 -- the resident form of the "composed" operator of csrc/joint_fit.hip (round 4; VERDICT r3 "Next" #3).
//
// The chain form spends 74-108 us per operator application in 8 dependent launches, two of them passes over the 33 MB of raw features
// (RN101, 480p, 5 augmented samples).  Here those features stay in VECTOR REGISTERS for the whole Gauss-Newton iteration, exactly like the
// memory of the filter problem in cg_persistent.hip, with ONE MORE DIMENSION: the Cin raw channels are cut into GROUPS of 96, and the c
// projected channels Z = w1 X (formed once per Gauss-Newton iteration by the GEMM kernel, before this launch) are one more group:
//
//   workgroup (group g, sample n, row part) = 8 waves x 12 channels, lane = x; it keeps its channels' rows [r0 - 2, r0 + R + 2) in registers.
//   One operator application  q = J^T J p + lam^2 p  with the direction p = (p1 (Cin x c, stored transposed), p2 (c x 9)):
//     every group holds its 3x3 "direction filter" F_g (96 x 9): raw groups the COMPOSED kernel F = p1 . w2 (the score has one channel, so
//     project-then-filter is one 3x3 filter over the raw features), the Z group F = p2;
//     1. partial scores of the own channels under F_g for the rows [r0 - 1, r0 + R]          -> global, write-through      | barrier A
//     2. every workgroup of (n, part) sums the NG partial maps itself (fixed order), applies the stencil t = sw (B s [- c])
//     3. weight gradient of the own channels against t from the SAME registers -> one 96 x 9 slab per workgroup            | barrier B
//     4. the KK = N x parts workgroups of a group each OWN a few of its channels: owner sums the KK slabs of its channels (fixed order) and
//        expands through w2:  q1[ch][c] = sum_tap G[ch][tap] w2[c][tap] + lam1 p1[ch][c]   (Z group: q2 = G + lam2 p2)
//   and the conjugate-gradient vectors (b, r, r_prev, p, q, x: 6 x 99 168 floats) are DISTRIBUTED the same way: each workgroup holds the
//   rows of its owned channels in LDS and performs the literal recurrences (optimizer.py:107-151, quirks of SURVEY App. B.8-10 included) on
//   them; the two dot products of an iteration are reduced through global memory (partials per workgroup, every workgroup sums all of
//   them in the same fixed order: identical scalars everywhere)                                                   | barriers C and D
//   The new direction p' = z + beta p is linear, so the owners publish the composed rows of z BEFORE barrier D, together with the partial
//   dots, and every workgroup forms F' = F_z + beta F locally afterwards: no fifth barrier.
// 4 grid barriers (3 on the last iteration) per operator application.  The barrier (XCD-hierarchical), the exchange protocol, the abort word
// and the phases over the resident rows are those of the filter problem's kernel: resident_grid.h.  A launch that times out writes NOTHING
// back (commit XOR abort: workgroup 0 claims the launch's abort word behind a final barrier) and bumps the sticky abort counter; the host
// then falls back to the chain form (model/optimizer.py).
// Results: the same algorithm as the chain form; dot products and slab sums have another (fixed) summation order and the new direction's
// composed kernel is formed as F_z + beta F instead of from p' itself: rounding-level differences, gated like the filter problem's
// persistent form (tests/test_round4_gpu.py).
#include "resident_grid.h"

namespace {

using namespace resident;          // NT, NWAVE, CPW, PW, FN (a group's direction filter / slab); the barrier, the sums and the phases
constexpr int GCH = CPW * NWAVE;   // 96 channels per group
constexpr int RMAX = 8;            // output rows per workgroup (8 + 4 halo rows x 12 channels = 144 feature registers per lane)
constexpr int XR = RMAX + 4;       // feature rows held per lane
constexpr int SR = RMAX + 2;       // score rows (stencil halo)

struct JParams {
  const float* X; const float* Z; const float* Bm; const float* cm; const float* sw;
  const float* w1T;                // (Cin, c): the projection, transposed (this launch's linearisation point)
  float* w1;                       // (c, Cin): updated in place at the end
  float* w2;                       // (c, 9): updated in place at the end
  float* vec; float* state;
  float* spart; float* slabs; float* Fbuf; float* dots;
  unsigned* bar; unsigned* hbar; unsigned* stats;
  int N, Cin, c, h, w, R, parts, NGr, cpo, own_stride, iters, has_p, apply_dff, fr, std_alpha;
  float dff, lam1, lam2, invM1, invM2, step;
  long long spin_limit;
};

// LDS carve-up (floats) behind the six owned vector slices (6 * own_stride floats, own_stride from the host)
constexpr int L_W2 = 0;                               // [96][9] filter.weight of this launch's linearisation point
constexpr int L_F = L_W2 + FN;                        // my group's direction filter
constexpr int L_FZ = L_F + FN;                        // scratch: composed z of my group / F of the carried direction
constexpr int L_GL = L_FZ + FN;                       // slab staging
constexpr int L_GX = L_GL + FN;                       // summed weight gradient of the owned channels [cpo][9] (<= 96 * 9)
constexpr int L_B = L_GX + FN;                        // [9][RMAX][64]
constexpr int L_C = L_B + 9 * RMAX * 64;              // [RMAX][64]
constexpr int L_S = L_C + RMAX * 64;                  // [SR][PW]
constexpr int L_T = L_S + SR * PW;                    // [RMAX][PW]
constexpr int L_RED = L_T + RMAX * PW;                // [NWAVE][SR][64]
constexpr int L_SRED = L_RED + NWAVE * SR * 64;       // 32
constexpr int L_FLAG = L_SRED + 32;                   // 4 ints
constexpr int L_FIXED = L_FLAG + 4;

__global__ __launch_bounds__(NT) void k_joint_run_persistent(const JParams P) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* w2l = lds + L_W2; float* vF = lds + L_F; float* vFz = lds + L_FZ; float* gl = lds + L_GL; float* gx = lds + L_GX;
  float (*Bl)[RMAX][64] = (float (*)[RMAX][64])(lds + L_B);
  float (*cl)[64] = (float (*)[64])(lds + L_C);
  float (*sl)[PW] = (float (*)[PW])(lds + L_S);
  float (*tl)[PW] = (float (*)[PW])(lds + L_T);
  float (*red)[SR][64] = (float (*)[SR][64])(lds + L_RED);
  float* sred = lds + L_SRED;
  int* sh_flag_p = (int*)(lds + L_FLAG);
  const int OS = P.own_stride;
  float* vb = lds + L_FIXED; float* vr = vb + OS; float* vrp = vr + OS; float* vp = vrp + OS; float* vq = vp + OS; float* vx = vq + OS;
  float* vw = vx + OS;             // the owned slice of the variables (7th slice)

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int G = gridDim.x, bid = blockIdx.x;
  const int KK = P.N * P.parts, NG = P.NGr + 1;
  const int g = bid / KK, k = bid - g * KK;
  const int n_s = k / P.parts, part = k - n_s * P.parts;
  const int r0 = part * P.R;
  const int R = min(P.R, P.h - r0);
  const int c = P.c, h = P.h, w = P.w, Cin = P.Cin;
  const bool zgrp = g == P.NGr;                       // the projected-feature group
  const int gbase = zgrp ? 0 : g * GCH;               // first channel of my group (in X or in Z)
  const int gcnt = zgrp ? c : min(GCH, Cin - gbase);  // channels of my group
  const int n1 = Cin * c;
  // owned channels (local to the group) and the owned slice of the vectors
  const int o0 = min(k * P.cpo, gcnt), o1 = min((k + 1) * P.cpo, gcnt), ocnt = o1 - o0;
  const int per = zgrp ? 9 : c;                       // vector elements per owned channel
  const int own = ocnt * per;
  const int vbase = zgrp ? n1 + o0 * 9 : (gbase + o0) * c;       // first global vector index of the owned slice (contiguous)
  const float lam = zgrp ? P.lam2 : P.lam1, invM = zgrp ? P.invM2 : P.invM1;
  GridBarrier gb(P.bar, P.hbar, P.stats, P.spin_limit, sh_flag_p);

  // ---- resident data ----
  float xr[CPW][XR];
  load_rows<RMAX>(xr, zgrp ? P.Z : P.X, zgrp ? (size_t)n_s * c : (size_t)n_s * Cin + gbase, gcnt, h, w, r0, P.R, lane, wid);
  load_maps<RMAX>(Bl, cl, sl, tl, P.Bm, P.cm, n_s, h, w, r0, R);
  for (int i = tid; i < FN; i += NT) { w2l[i] = i < c * 9 ? P.w2[i] : 0.f; vF[i] = 0.f; vFz[i] = 0.f; gx[i] = 0.f; }
  for (int i = tid; i < OS; i += NT) {
    const bool on = i < own;
    // variables of the owned slice: raw groups rows of w1T (Cin x c), the Z group rows of w2 (c x 9)
    vw[i] = on ? (zgrp ? P.w2[o0 * 9 + i] : P.w1T[(size_t)(gbase + o0) * c + i]) : 0.f;
    vp[i] = (on && P.has_p) ? P.vec[(size_t)3 * (n1 + c * 9) + vbase + i] : 0.f;
    vrp[i] = (on && P.has_p) ? P.vec[(size_t)2 * (n1 + c * 9) + vbase + i] : 0.f;
    vb[i] = vr[i] = vq[i] = vx[i] = 0.f;
  }
  const float swn = P.sw[n_s];
  if (!gb.join()) return;                             // XCD registration behind ONE flat barrier; ends in a workgroup barrier (LDS above is set up)

  // ---- composed rows of an owned vector slice -> Fbuf[slot][g][(o0 + chl) * 9 + tap]  (raw groups: v . w2; Z group: v itself) ----
  auto publish_compose = [&](const float* v, int slot) {
    float* dst = P.Fbuf + ((size_t)slot * NG + g) * FN + o0 * 9;
    for (int e = tid; e < ocnt * 9; e += NT) {
      float s = 0.f;
      if (zgrp) s = v[e];
      else {
        const int chl = e / 9, tap = e - chl * 9;
        const float* vrow = v + chl * c;
        for (int cc = 0; cc < c; ++cc) s += vrow[cc] * w2l[cc * 9 + tap];           // fixed order
      }
      st_wt(dst + e, s);
    }
  };
  auto read_F = [&](float* dstl, int slot) {           // my group's published filter -> LDS (zeros beyond the group's channels)
    const float* src = P.Fbuf + ((size_t)slot * NG + g) * FN;
    for (int i = tid; i < FN; i += NT) dstl[i] = i < gcnt * 9 ? ld_l2(src + i) : 0.f;
  };
  // ---- global sums of two per-workgroup partials (every workgroup sums all of them in the same order) ----
  auto publish_dots = [&](float a, float b, int slot) {
    if (tid == 0) { st_wt(P.dots + ((size_t)slot * G + bid) * 2, a); st_wt(P.dots + ((size_t)slot * G + bid) * 2 + 1, b); }
  };
  auto sum_dots = [&](float& a, float& b, int slot) {
    float sa = 0.f, sb = 0.f;
    if (wid == 0) {
      for (int q = lane; q < G; q += 64) { sa += ld_l2(P.dots + ((size_t)slot * G + q) * 2); sb += ld_l2(P.dots + ((size_t)slot * G + q) * 2 + 1); }
      sa = wave_sum_to63(sa); sb = wave_sum_to63(sb);
      if (lane == 63) { sred[0] = sa; sred[1] = sb; }
    }
    __syncthreads();
    a = sred[0]; b = sred[1];
    __syncthreads();
  };

  // ---- one operator application with the group filters in vF: vq (owned slice) <- (J^T (sw (B s - c?)))_owned + lam v_owned ----
  auto apply = [&](const float* v_own, bool with_c, bool scores_on) -> bool {
    // 1. partial scores of the own channels: three column partials per score row
    float* sp = P.spart + ((size_t)k * NG + g) * (SR * 64);
    if (scores_on) {
      partial_scores<RMAX>(xr, vF, red, [&](int i, float s) { st_wt(sp + i, s); });          // (vF: zero beyond the group's channels)
    } else {
      for (int i = tid; i < SR * 64; i += NT) st_wt(sp + i, 0.f);
    }
    if (!gb.sync()) return false;                                                       // ---- barrier A
    // 2. the full score rows of (n, part): sum of the NG partial maps, fixed order; then the stencil
    for (int i = tid; i < SR * 64; i += NT) {
      const int jj = i >> 6, x = i & 63;
      const int yy = r0 - 1 + jj;
      float s = 0.f;
      const float* base = P.spart + (size_t)k * NG * (SR * 64) + i;
      for (int q = 0; q < NG; ++q) s += ld_l2(base + (size_t)q * (SR * 64));
      sl[jj][x + 1] = (x < w && (unsigned)yy < (unsigned)h && jj < R + 2) ? s : 0.f;
    }
    __syncthreads();
    stencil<RMAX>(Bl, cl, sl, tl, R, w, with_c, swn);
    // 3. weight gradient of the own channels from the resident rows
    weight_gradient<RMAX>(xr, tl, gl, P.slabs + ((size_t)g * KK + k) * FN);
    if (!gb.sync()) return false;                                                       // ---- barrier B
    // 4. owners: sum of the KK slabs of the owned channels (one wave per element, fixed order), then the expansion through w2
    for (int e0 = wid; e0 < ocnt * 9; e0 += NWAVE) {
      const int e = o0 * 9 + e0;
      float s = 0.f;
      for (int q = lane; q < KK; q += 64) s += ld_l2(P.slabs + ((size_t)g * KK + q) * FN + e);
      s = wave_sum_to63(s);
      if (lane == 63) gx[e0] = s;
    }
    __syncthreads();
    for (int i = tid; i < OS; i += NT) {
      float qv = 0.f;
      if (i < own) {
        if (zgrp) qv = gx[i];
        else {
          const int chl = i / c, cc = i - chl * c;
          const float* gr = gx + chl * 9;
          const float* wr = w2l + cc * 9;
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) qv += gr[tap] * wr[tap];
        }
        qv += lam * v_own[i];
      }
      vq[i] = qv;
    }
    __syncthreads();
    return true;
  };

  // ---- right-hand side b = -(J^T f(w) + lam^2 w): the scores are Z * w2 (the Z group alone contributes, with F = w2) ----
  if (zgrp) { for (int i = tid; i < FN; i += NT) vF[i] = w2l[i]; }
  if (P.has_p) publish_compose(vp, 1);                 // composed kernel of the carried direction (slot 1), read behind the barrier below
  __syncthreads();
  if (!apply(vw, true, zgrp)) return;
  // r = b; z = M^-1 r; rho' = <r,z>; rho2 = <r_prev,z>   (optimizer.py:107-130)
  float rho_cur;
  {
    float d0 = 0.f, d1 = 0.f;
    for (int i = tid; i < OS; i += NT) {
      const float bv = -vq[i];
      vb[i] = bv; vr[i] = bv;
      const float z = bv * invM;
      d0 += bv * z;
      if (P.has_p && !P.fr) d1 += vrp[i] * z;
      vx[i] = z;                                       // (vx is free until the first step: staging of z for the compose below)
    }
    bsum2(d0, d1, sred);
    publish_dots(d0, d1, 0);
    publish_compose(vx, 0);                            // composed rows of z (slot 0)
    if (!gb.sync()) return;                                                              // ---- barrier C'
    sum_dots(d0, d1, 0);
    float beta = 0.f;
    if (P.has_p) {
      float rho1 = P.state[0];
      if (P.apply_dff) rho1 = rho1 / P.dff;
      const float vv = P.fr ? d0 / rho1 : (d0 - d1) / rho1;
      beta = (vv < 0.f) ? 0.f : vv;
    }
    read_F(vFz, 0);
    if (P.has_p) read_F(vF, 1);
    __syncthreads();
    for (int i = tid; i < FN; i += NT) vF[i] = P.has_p ? vFz[i] + vF[i] * beta : vFz[i];
    for (int i = tid; i < OS; i += NT) {
      const float z = vr[i] * invM;
      vp[i] = P.has_p ? (z + vp[i] * beta) : z;
      vx[i] = 0.f;
    }
    rho_cur = d0;
    __syncthreads();
  }
  float alpha = 0.f, beta_last = 0.f, rho_prev = P.state[0];
  for (int it = 0; it < P.iters; ++it) {
    if (!apply(vp, false, true)) return;
    const bool first = it == 0, last = it == P.iters - 1;
    float pq = 0.f, pr = 0.f;
    for (int i = tid; i < OS; i += NT) { pq += vp[i] * vq[i]; pr += vp[i] * vr[i]; }
    bsum2(pq, pr, sred);
    publish_dots(pq, pr, 1);
    if (!gb.sync()) return;                                                              // ---- barrier C
    sum_dots(pq, pr, 1);
    alpha = P.std_alpha ? rho_cur / pq : pr / pq;
    float rn_ = 0.f, r2_ = 0.f;
    for (int i = tid; i < OS; i += NT) {
      const float rv = vr[i], pv = vp[i];
      vrp[i] = rv;
      vx[i] = first ? pv * alpha : vx[i] + pv * alpha;
      float rn = rv;
      if (!last) { rn = rv - vq[i] * alpha; vr[i] = rn; }
      const float z = rn * invM;
      rn_ += rn * z;
      r2_ += rv * z;
    }
    rho_prev = rho_cur;
    if (!last) {
      // z of the owned slice, staged in vq (its content is consumed): composed rows published together with the partial dots
      for (int i = tid; i < OS; i += NT) vq[i] = vr[i] * invM;
      bsum2(rn_, r2_, sred);
      publish_dots(rn_, r2_, 0);
      publish_compose(vq, 0);
      if (!gb.sync()) return;                                                            // ---- barrier D
      sum_dots(rn_, r2_, 0);
      const float vv = P.fr ? rn_ / rho_cur : (rn_ - r2_) / rho_cur;
      beta_last = (vv < 0.f) ? 0.f : vv;
      read_F(vFz, 0);
      __syncthreads();
      for (int i = tid; i < FN; i += NT) vF[i] = vFz[i] + vF[i] * beta_last;
      for (int i = tid; i < OS; i += NT) vp[i] = vq[i] + vp[i] * beta_last;
      rho_cur = rn_;
    }
    __syncthreads();
  }
  // ---- write back: every workgroup its owned slices, behind a final barrier, and only if the launch COMMITS (protocol at grid_sync) ----
  if (!gb.sync()) return;
  if (tid == 0) {
    unsigned st;
    if (bid == 0) st = claim_commit(gb.abort_flag(), P.stats);
    else {
      // wait for workgroup 0's decision (it is resident and a few instructions away) -- bounded like every other wait
      const long long t0 = wall_clock64();
      while ((st = __hip_atomic_load(gb.abort_flag(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u) {
        __builtin_amdgcn_s_sleep(1);
        if (wall_clock64() - t0 > P.spin_limit) { st = give_up_or_committed(gb.abort_flag(), P.stats) ? 2u : 1u; break; }
      }
    }
    sh_flag_p[0] = st == 2u ? 1 : 0;
  }
  __syncthreads();
  if (!sh_flag_p[0]) return;
  const size_t n = (size_t)n1 + c * 9;
  for (int i = tid; i < own; i += NT) {
    P.vec[0 * n + vbase + i] = vb[i];
    P.vec[1 * n + vbase + i] = vr[i];
    P.vec[2 * n + vbase + i] = vrp[i];
    P.vec[3 * n + vbase + i] = vp[i];
    P.vec[4 * n + vbase + i] = vq[i];
    P.vec[5 * n + vbase + i] = vx[i];
    const float nv = vw[i] + P.step * vx[i];
    if (zgrp) P.w2[o0 * 9 + i] = nv;
    else { const int chl = i / c, cc = i - chl * c; P.w1[(size_t)cc * Cin + gbase + o0 + chl] = nv; }      // un-transposed: project.weight is (c, Cin)
  }
  if (bid == 0 && tid == 0) {
    P.state[0] = P.iters > 0 ? rho_prev : P.state[0];
    P.state[4] = rho_cur;
    P.state[1] = alpha;
    P.state[2] = beta_last;
  }
}

}  // namespace

extern "C" {

// Workgroups of the resident form of the joint problem (0: the problem does not fit).  out4 = {parts, rows per part, owned channels per
// workgroup, floats of one owned vector slice in LDS}.
int frtm_joint_persistent_plan(int N, int Cin, int c, int h, int w, int* out4) {
  if (N < 1 || Cin < 1 || c < 1 || c > GCH || w < 1 || w > 64 || h < 1) return 0;
  const int budget = resident_budget();
  const int NG = ceil_div(Cin, GCH) + 1;
  const int min_parts = ceil_div(h, RMAX);
  if ((long)NG * N * min_parts > budget) return 0;
  int parts = budget / (NG * N);
  if (parts > h) parts = h;
  if (parts < min_parts) parts = min_parts;
  int R = ceil_div(h, parts);
  parts = ceil_div(h, R);
  const int KK = N * parts;
  const int cpo = ceil_div(GCH, KK);
  const int own_stride = cpo * (c > 9 ? c : 9);
  if ((size_t)(L_FIXED + 7 * own_stride) * 4 > 160 * 1024) return 0;
  if (out4) { out4[0] = parts; out4[1] = R; out4[2] = cpo; out4[3] = own_stride; }
  return NG * N * parts;
}

// Scratch (floats) of a launch: partial score rows, slabs, two filter slots, two dot slots.
size_t frtm_joint_persistent_scratch(int N, int Cin, int c, int h, int w) {
  int o[4];
  const int G = frtm_joint_persistent_plan(N, Cin, c, h, w, o);
  if (G <= 0) return 0;
  const int NG = ceil_div(Cin, GCH) + 1, KK = N * o[0];
  return (size_t)KK * NG * SR * 64 + (size_t)NG * KK * FN + (size_t)2 * NG * FN + (size_t)2 * G * 2 + 64;
}

int frtm_joint_run_persistent(const float* X, const float* Z, const float* Bm, const float* cm, const float* sw, int N, int Cin, int c, int h, int w,
                              const float* w1T, float* w1, float* w2, float* vec, float* state, float* scratch, unsigned* bar, unsigned* hbar,
                              int iters, int has_p, int apply_dff, int fletcher_reeves, int standard_alpha, float dff, float lam1, float lam2,
                              float invM1, float invM2, float step, unsigned* stats, int debug_abort, frtm_stream_t stream) {
  FRTM_CHECK_ARG(X && Z && Bm && cm && sw && w1T && w1 && w2 && vec && state && scratch && bar && iters >= 0, "frtm_joint_run_persistent: bad argument");
  int o[4];
  const int G = frtm_joint_persistent_plan(N, Cin, c, h, w, o);
  FRTM_CHECK_ARG(G > 0, "frtm_joint_run_persistent: problem (N=%d, Cin=%d, c=%d, %dx%d) does not fit the resident form", N, Cin, c, h, w);
  JParams P;
  P.X = X; P.Z = Z; P.Bm = Bm; P.cm = cm; P.sw = sw; P.w1T = w1T; P.w1 = w1; P.w2 = w2; P.vec = vec; P.state = state;
  const int NG = ceil_div(Cin, GCH) + 1, KK = N * o[0];
  P.spart = scratch;
  P.slabs = P.spart + (size_t)KK * NG * SR * 64;
  P.Fbuf = P.slabs + (size_t)NG * KK * FN;
  P.dots = P.Fbuf + (size_t)2 * NG * FN;
  P.bar = bar; P.hbar = hbar; P.stats = stats;
  P.N = N; P.Cin = Cin; P.c = c; P.h = h; P.w = w; P.R = o[1]; P.parts = o[0]; P.NGr = NG - 1; P.cpo = o[2]; P.own_stride = o[3];
  P.iters = iters; P.has_p = has_p; P.apply_dff = apply_dff; P.fr = fletcher_reeves; P.std_alpha = standard_alpha;
  P.dff = dff; P.lam1 = lam1; P.lam2 = lam2; P.invM1 = invM1; P.invM2 = invM2; P.step = step;
  P.spin_limit = resident_spin_limit(debug_abort);
  const size_t lds = (size_t)(L_FIXED + 7 * o[3]) * 4;
  static size_t attr_lds = 0;
  if (lds > attr_lds) {
    FRTM_HIP(hipFuncSetAttribute((const void*)k_joint_run_persistent, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_lds = lds;
  }
  if (int e = resident_reset_words(bar, hbar, (hipStream_t)stream)) return e;
  k_joint_run_persistent<<<G, NT, lds, (hipStream_t)stream>>>(P);
  FRTM_LAUNCH_CHECK();
  return FRTM_OK;
}

}  // extern "C"
