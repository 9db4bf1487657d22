/* libfrtm_hip -- C ABI of the MI355X-native FRTM hot path (gfx950 HIP kernels).
 *
 * The reference (andr345/frtm-vos) is pure Python on PyTorch and has NO native interface for
 * this path (its only native file, lib/_npp/nppig.cpp, wraps NVIDIA NPP image warps for the
 * augmenter).  Every device op of the hot path is an ATen/cuDNN launch issued from Python.
 * This header therefore defines the boundary a maintainer of the reference would bind
 * (ctypes stub: INTEGRATION.md); each entry point cites the reference code it replaces.
 *
 * Conventions
 *  - all pointers are DEVICE pointers unless the name ends in _host; tensors are dense fp32,
 *    NCHW, exactly as PyTorch lays them out (tensor.data_ptr()).
 *  - every function takes a hipStream_t (as void*) and never synchronises.
 *  - return value: 0 = ok, <0 = error; frtm_last_error() returns the message (thread local).
 *  - nothing here allocates per call; scratch buffers are passed in (sizes documented).
 */
#ifndef FRTM_HIP_H
#define FRTM_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

typedef void* frtm_stream_t;            /* hipStream_t */
typedef struct frtm_backbone frtm_backbone_t;

const char* frtm_last_error(void);
int frtm_version(void);
/* Device properties of the current device: out[0]=CU count, out[1]=gfx arch number (950),
 * out[2]=LDS bytes per workgroup, out[3]=wavefront size. */
int frtm_device_info(int* out4_host);

/* ------------------------------------------------------------------------------------------
 * Target model ("discriminator"), per-frame pieces
 * ------------------------------------------------------------------------------------------ */

/* Discriminator.compute_pixel_weights, method 'hinge' (model/discriminator.py:107-152).
 * y: (n,1,H,W) labels in {0,1}, uint8 if y_is_u8 else fp32.  out: (n,1,H,W) fp32.
 * tf < 0 selects "no weighting" (all ones, :114-115).  scratch: >= n*FRTM_PX_PARTS floats. */
#define FRTM_PX_PARTS 32
int frtm_pixel_weights(const void* y, int y_is_u8, int n, int H, int W, float tf,
                       float* out, float* scratch, frtm_stream_t stream);

/* Low-resolution normal equations of one memory sample (replaces storing the hi-res label and
 * pixel-weight maps of model/memory.py:15-16 and the hi-res work of DiscriminatorLoss.__call__,
 * model/discriminator.py:45-49, inside the CG loop):
 *     B = U^T diag(pw^2) U   (a 3x3 stencil on the h x w grid, 9 maps)      c = U^T (pw^2 * label)
 * with U = bilinear up-sampling (h,w)->(H,W), align_corners=False, and pw the hinge pixel weight
 * of ys = (label > 0.5) (discriminator.py:217-218).  labels: (n,1,H,W) uint8 or fp32 (soft).
 * Results go to slots slot..slot+n-1 of Bmem (cap,9,h,w) and cmem (cap,h,w); if slot_dev != NULL
 * the first slot index is read from that device int32 (Memory.update's argmin, memory.py:80),
 * otherwise slot_host is used.  tf < 0: pw = 1.  pw != NULL: explicit (n,1,H,W) pixel weights are used
 * instead of the hinge rule (Memory.update's generic signature, memory.py:59).
 * scratch: >= n*FRTM_PX_PARTS floats.  px_count_dev: optional device int32[n] with the number of label pixels > 0.5 per
 * sample (the caller often has it already: frtm_count_above for the early-out test); NULL: it is computed here. */
int frtm_normal_build(const void* labels, int labels_is_u8, const float* pw, int n, int H, int W, int h, int w,
                      float tf, const int* slot_dev, int slot_host, float* Bmem, float* cmem,
                      float* scratch, const int* px_count_dev, frtm_stream_t stream);

/* Memory.update (memory.py:59-92) for a WINDOW of W frames in three launches: the W slot choices one after the other on the device
 * (sample weights updated in between exactly as W calls of frtm_memory_next_slot would; counts[f * count_stride] < min_count skips
 * frame f), the W feature copies (features: (W, len) dense), the W low-resolution normal equations from float label planes
 * `label_stride` elements apart (hinge pixel weights from the same counts).  slots: device int[W] scratch, left filled. */
int frtm_memory_update_window(float* sw, int cap, float lr, int num_samp_is_zero, int* state, const int* counts, int count_stride,
                              int min_count, int W, int* slots, const float* features, float* samples, int len, const float* labels,
                              size_t label_stride, int H, int Wd, int h, int w, float tf, float* Bmem, float* cmem, float* scratch,
                              frtm_stream_t stream);
/* Memory.update_sample_weights (model/memory.py:65-92) on the device, no host sync.
 * sw: (cap) sample weights, updated in place.  state: device int32[4] = {previous_replace_ind or -1,
 * replace index written by this call, number of inserts performed so far (incremented here), number of inserts skipped
 * through count_dev (incremented here)}.  num_samp_is_zero / lr as in the reference.
 * count_dev != NULL: device int32 holding the number of mask pixels > 0.5; if it is < min_count the call leaves the
 * weights untouched and writes slot -1, which makes frtm_memory_insert / frtm_normal_build no-ops: the early-out of
 * Discriminator.update (discriminator.py:214) without a host sync. */
int frtm_memory_next_slot(float* sw, int cap, float lr, int num_samp_is_zero, int* state,
                          const int* count_dev, int min_count, frtm_stream_t stream);

/* Copy one sample (len floats) into slot state[1] of a (cap,len) buffer (Memory.insert_at, memory.py:50-57). */
int frtm_memory_insert(const float* src, float* dst_base, int len, const int* slot_dev, frtm_stream_t stream);

/* 3x3 filter scores (Discriminator.filter, model/discriminator.py:82,205; C1 of SURVEY 2.3):
 * out[n,y,x] (+)= sum_c sum_{dy,dx} X[n,c,y+dy-1,x+dx-1] * f[c,dy,dx].  X (N,C,h,w), f (1,C,3,3). */
int frtm_filter_scores(const float* X, const float* f, int N, int C, int h, int w,
                       float* out, int accumulate, frtm_stream_t stream);

/* frtm_filter_scores with the channels split over `splits` groups of workgroups (maps at most 64 wide): partial map k
 * (partial + k*N*h*w) holds the sum over channel group k; for FEW samples with MANY channels (raw trunk features of the
 * first-frame problem).  frtm_stencil_sum is frtm_stencil over the sum of nsum such partial maps (fixed summation order). */
int frtm_filter_scores_split(const float* X, const float* f, int N, int C, int h, int w, int splits, float* partial, frtm_stream_t stream);
int frtm_stencil_sum(const float* B, const float* c, const float* sw, const float* partials, int nsum, int N, int h, int w, float* t,
                     frtm_stream_t stream);
/* t[n,i,j] = sw[n] * ( sum_{di,dj} B[n,(di,dj),i,j] * s[n,i+di,j+dj]  -  (c ? c[n,i,j] : 0) ).
 * This is U^T W^2 (U s - y) of the reference residual (discriminator.py:47-49) in low-res form. */
int frtm_stencil(const float* B, const float* c, const float* sw, const float* s, int N, int h, int w,
                 float* t, frtm_stream_t stream);

/* Filter weight gradient as partial slabs (the conv backward of optimizer.py:84,155-157):
 *   sum over part of partial[n*parts + part, c*9+dy*3+dx] = sum_{y,x} X[n,c,y+dy-1,x+dx-1] * t[n,y,x].
 * `parts` >= 1 splits each sample's pixels over that many blocks (more parallelism when N is small);
 * partial: float[N*parts][C*9].  frtm_filter_wgrad_parts() returns the split the library recommends for (N, C). */
int frtm_filter_wgrad(const float* X, const float* t, int N, int C, int h, int w, int parts,
                      float* partial, frtm_stream_t stream);
int frtm_filter_wgrad_parts(int N, int C);
/* ... with the number of pixels of a map taken into account (large maps are cut into more parts). */
int frtm_filter_wgrad_parts_hw(int N, int C, int hw);

/* The same with the stencil fused in: t = sw * (B s - c) is formed inside the kernel from the scores s (c may be NULL). */
int frtm_filter_wgrad_stencil(const float* X, const float* s, const float* B, const float* c, const float* sw,
                              int N, int C, int h, int w, float* partial, frtm_stream_t stream);

/* Input gradient of the 3x3 filter: D[n,c,y,x] = sum_{dy,dx} f[c,dy,dx] * t[n,y-dy+1,x-dx+1].
 * pix_major != 0 writes D as (n, h*w, C) instead of (n, C, h*w). */
int frtm_filter_igrad(const float* t, const float* f, int N, int C, int h, int w,
                      float* D, int pix_major, frtm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conjugate-gradient vector steps (model/optimizer.py:98-153), scalars stay on the device.
 * Vectors are flat fp32 of length n = n1 + n2 (two parameter tensors; n2 may be 0); the
 * preconditioner M1 (discriminator.py:63-64) divides part k by diagM[k].
 * state: device float[8]: [0]=rho [1]=alpha [2]=beta [3]=pq [4]=rho_new [5]=rho2.
 * partial: device float[>= 4*FRTM_CG_BLOCKS] (two banks of per-block dot partials).
 * ------------------------------------------------------------------------------------------ */
#define FRTM_CG_BLOCKS 64
/* q = sign * ( sum_k slabs[k*stride + i] + lam2 * p[i] ),  i < len   (sign = +1 / -1) */
int frtm_vec_reduce_slabs(const float* slabs, int nslab, int stride, int len, float lam2, const float* p,
                          float sign, float* q, frtm_stream_t stream);
/* r = b; partial dots of rho_new=<r,M^-1 r> and (has_p) rho2=<r_prev,M^-1 r>   (optimizer.py:107-117) */
int frtm_cg_begin(const float* b, float* r, const float* r_prev, int n1, int n2, float invM1, float invM2,
                  int has_p, float* partial, frtm_stream_t stream);
/* beta = clamp((rho_new-rho2)/rho1, 0); p = z + beta p  (or p = z when !has_p); rho <- rho_new.
 * apply_dff != 0: rho1 = rho / dff first (optimizer.py:102-105). */
int frtm_cg_direction(const float* r, float* p, int n1, int n2, float invM1, float invM2, int has_p,
                      int apply_dff, int fletcher_reeves, float dff, float* state, const float* partial,
                      frtm_stream_t stream);
/* partial dots of <p,q> (optimizer.py:133) and, if r != NULL, <p,r> (non-standard alpha, :138) */
int frtm_cg_pq(const float* p, const float* q, const float* r, int n, float* partial, frtm_stream_t stream);
/* alpha = rho/pq; r_prev = r; x = first ? alpha p : x + alpha p; if(!last) r -= alpha q; then the
 * partial dots for the next direction (optimizer.py:135-151,113-127). */
int frtm_cg_update(float* x, float* r, float* r_prev, const float* p, const float* q, int n1, int n2,
                   float invM1, float invM2, int first, int last, int standard_alpha, float* state,
                   float* partial, frtm_stream_t stream);
/* Fused glue of the JOINT first-frame problem (reference discriminator.py:165-176): fewer dependent launches per operator
 * application (csrc/joint_fit.hip).
 *   frtm_filter_scores2   out (N,1,h,w) = X1 * f1 + X2 * f2   (two 3x3 score passes in one launch; X (N,C,h,w), f (1,C,3,3))
 *   frtm_joint_mid        t = sw (B s [- cm]) formed per block in LDS, then BOTH the filter weight-gradient slabs of Z
 *                         (partial: (N*parts, C*9), like frtm_filter_wgrad) and the input gradient D (N,h*w,C) pixel-major
 *                         (like frtm_filter_igrad(..., pix_major=1)); cm may be NULL
 *   frtm_joint_q_pq       q[:n1] = sign (g1 + lam1 p1), q[n1:] = sign (sum_k slabs[k*stride + i] + lam2 p2); if partial != NULL
 *                         also the FRTM_CG_BLOCKS partials of <p,q> (and <p,r> when r != NULL) in frtm_cg_pq's layout */
int frtm_filter_scores2(const float* X1, const float* f1, const float* X2, const float* f2, int N, int C, int h, int w, float* out,
                        frtm_stream_t stream);
int frtm_joint_mid(const float* s, const float* Bm, const float* cm, const float* sw, const float* Z, const float* w2, int N, int C,
                   int h, int w, int parts, float* partial, float* D, frtm_stream_t stream);
int frtm_joint_q_pq(const float* g1, int n1, float lam1, const float* slabs, int nslab, int stride, int n2, float lam2, const float* p1,
                    const float* p2, float sign, float* q, const float* r, float* partial, frtm_stream_t stream);
/* Fused launches of the composed form.  frtm_joint_scores_composed: partial score maps 0..splits-1 = channel groups of X under K,
 * map `splits` = Z under p2 (partial: (splits+1, N, h, w); sum them with frtm_stencil_sum).  frtm_joint_q_pq_composed: q1 as
 * frtm_joint_expand, q2 = sign * (sum of the nslab slabs of the projected features' gradient + lam2 p2) and, if partial != NULL,
 * the FRTM_CG_BLOCKS per-block partials of <p,q> (and <p,r> if r != NULL) that frtm_cg_update sums. */
int frtm_joint_scores_composed(const float* X, const float* K, int Cx, const float* Z, const float* p2, int Cz, int N, int h, int w,
                               int splits, float* partial, frtm_stream_t stream);

/* Wide feature maps (64 < w <= 256, w % 4 == 0: the 45 x 80 / 68 x 120 maps of 720p / 1080p), csrc/wide_maps.hip (round 5): the two HBM-bound
 * passes of an operator application in strip form (a lane owns 4 columns x 8 rows, dwordx4 rows, neighbours by DPP).
 *   frtm_wide_parts       row blocks the strip forms cut an h x w map into (= slabs per sample of frtm_wgrad_wide); 0 = maps the forms do not take
 *   frtm_scores_wide      frtm_joint_scores_composed's contract (reference discriminator.py:45-50 through the composed kernel)
 *   frtm_wgrad_wide       frtm_filter_wgrad's contract with parts = frtm_wide_parts(h, w): partial float[N*parts][C*9] */
int frtm_wide_parts(int h, int w);
int frtm_scores_wide(const float* X, const float* K, int Cx, const float* Z, const float* p2, int Cz, int N, int h, int w,
                     int splits, float* partial, frtm_stream_t stream);
int frtm_wgrad_wide(const float* X, const float* t, int N, int C, int h, int w, float* partial, frtm_stream_t stream);
int frtm_joint_q_pq_composed(const float* GX, int nslabX, int Cin, int c, const float* w2, float lam1, const float* slabs, int nslab,
                             int stride, int n2, float lam2, const float* p1, const float* p2, float sign, float* q, const float* r,
                             float* partial, frtm_stream_t stream);
/* Composed form of the joint problem's projection part (the score has ONE channel, so project-then-filter is a single 3x3
 * filter over the raw features): K[ci][tap] = sum_c p1[ci][c] w2[c][tap] (p1 as (Cin,c), w2 as (c,9), c <= 128) -- use K with
 * frtm_filter_scores on the raw features -- and, for the gradient, q1[ci][c] = sign * ( sum_tap (sum_slab G[slab][ci][tap])
 * w2[c][tap] + lam2 p1[ci][c] ) from the per-sample slabs G that frtm_filter_wgrad leaves for the raw features against t.
 * Replaces the two Cin x c x pixels GEMMs of an operator application (discriminator.py:165-176 through autograd). */
int frtm_joint_compose(const float* p1, const float* w2, int Cin, int c, float* K, frtm_stream_t stream);
int frtm_joint_expand(const float* G, int nslab, const float* w2, int Cin, int c, float lam2, const float* p1, float sign, float* q1,
                      frtm_stream_t stream);

/* One whole Gauss-Newton iteration of the FILTER problem (reference optimizer.py:77-153 on the problem of
 * discriminator.py:187-196) as ONE persistent launch: right-hand side b = -(J^T f(w2) + lam2 w2), `iters` CG steps with the
 * literal recurrences (carried p / r_prev / rho as in frtm_cg_begin / _direction / _step_small), then w2 += step * delta.
 * The sample features X (N,c,h,w) are read once and stay in registers; Bm (N,9,h,w), cm (N,h,w), sw (N) are the memory's
 * low-resolution normal equations and sample weights.  vec: the solver's 6*n floats {b,r,r_prev,p,q,delta}, n = 9c;
 * state: float[8] as above; slabs: >= 256*864 floats, qbuf: >= 864 + 256 floats, bar: unsigned[4] (bar[0..2]: arrivals / spare / abort flag
 * of ONE launch, zeroed by a memset node in front of every launch; bar[3] != 0: workgroup 0 also writes phase time stamps to qbuf[864..]).
 * A launch whose workgroups cannot all become resident within the spin time-out (4 ms) ABORTS: x, vec and state stay untouched and
 * stats[2] (see the guarded entry) is incremented; the caller re-runs the solve in the multi-kernel form.
 * frtm_cg_persistent_plan returns the number of workgroups (0 = shape not supported: w > 64, c > 96, or N*ceil(h/10) above the
 * resident budget = 15/16 of the current device's CUs, 240 on an MI355X); all of them must be resident at once: never run two of these
 * launches concurrently on one GPU. */
#define FRTM_HBAR_WORDS 288   /* unsigned words of `hbar`, the XCD-hierarchical barrier's state, in both resident solvers (layout: csrc/resident_grid.h) */
int frtm_cg_persistent_plan(int N, int c, int h, int w, int* parts_out, int* rows_out);
int frtm_cg_run_persistent(const float* X, const float* Bm, const float* cm, const float* sw, int N, int c, int h, int w,
                           float* w2, float* vec, float* state, float* slabs, float* qbuf, unsigned* bar,
                           int iters, int has_p, int apply_dff, int fletcher_reeves, int standard_alpha, float dff,
                           float lam2, float invM, float step, frtm_stream_t stream);
/* The same launch with the reference's early-out (discriminator.py:214, "fewer than 10 mask pixels above 0.5: no update") decided on
 * the DEVICE: guard_count (device int32, e.g. one element of frtm_count_above's output) < guard_min -> the launch returns without
 * touching anything.  stats (device unsigned[4], optional): with count_run != 0, [0] += 1 per completed launch, [1] += 1 per guarded
 * early-out; [2] += 1 per ABORTED launch (always).  debug_abort != 0 forces the time-out (tests of the caller's fallback).  The host
 * never waits for the pixel count, so a tracking loop enqueues whole sequences without a device->host read.
 * hbar (device unsigned[FRTM_HBAR_WORDS], optional): state of the XCD-hierarchical grid barrier (zeroed by the launch); NULL: flat barrier. */
int frtm_cg_run_persistent_guarded(const float* X, const float* Bm, const float* cm, const float* sw, int N, int c, int h, int w,
                                   float* w2, float* vec, float* state, float* slabs, float* qbuf, unsigned* bar,
                                   int iters, int has_p, int apply_dff, int fletcher_reeves, int standard_alpha, float dff,
                                   float lam2, float invM, float step, const int* guard_count, int guard_min, unsigned* stats,
                                   int count_run, int debug_abort, unsigned* hbar, frtm_stream_t stream);
/* The same early-out for solves that run as a CHAIN of launches (maps wider than 64 columns, memories beyond the resident budget,
 * the fallback after an aborted persistent launch): the caller snapshots the solver's device state before the chain
 * (mode 0: dst <- src, n floats) and rolls it back after it when the guard says the update should not have happened
 * (mode 1: dst <- src only if *guard_count < guard_min; stats[1] += 1 then, else stats[0] += 1, when stats != NULL and count != 0).
 * The work of a skipped solve is wasted (rare: an object with fewer than 10 pixels on a re-solve frame) -- nothing is read by the host. */
int frtm_guarded_copy(float* dst, const float* src, int n, const int* guard_count, int guard_min, int mode, unsigned* stats, int count,
                      frtm_stream_t stream);
/* One CG iteration's vector work for n <= 1024 in a single workgroup (the 864-element filter problem): slab reduce
 * (q = sum_k slabs[k*stride+i] + lam2 p), <p,q>, alpha, r_prev/x/r updates, and -- unless `last` -- the next direction
 * (beta, p, rho).  Same order of operations as optimizer.py:113-151; replaces frtm_vec_reduce_slabs + frtm_cg_pq +
 * frtm_cg_update + frtm_cg_direction on that problem. */
int frtm_cg_step_small(const float* slabs, int nslab, int stride, float lam2, float* x, float* r, float* r_prev,
                       float* p, float* q, int n, float invM, int first, int last, int standard_alpha,
                       int fletcher_reeves, float* state, frtm_stream_t stream);
/* ------------------------------------------------------------------------------------------
 * Round 4: one Gauss-Newton iteration of the JOINT first-frame problem (reference discriminator.py:154-199 on optimizer.py:77-153) as ONE
 * resident launch (csrc/joint_persistent.hip): the raw features X (N, Cin, h, w) and the projected features Z (N, c, h, w) = w1 X stay in
 * registers, channel group by channel group, for the right-hand side, `iters` CG steps and the step x += step * delta.
 * plan: number of workgroups (0 = does not fit: w > 64, c > 96, too many samples); out4 = {row parts, rows per part, owned channels per
 * workgroup, floats per owned vector slice}.  scratch: floats of exchange scratch a launch needs.
 * w1T (Cin, c) = project.weight transposed at the linearisation point (input); w1 (c, Cin) and w2 (c, 9) are UPDATED in place; vec / state
 * as in frtm_cg_*: vec = [b, r, r_prev, p, q, delta] x (Cin c + 9 c) with the projection part stored transposed, state[0] = rho ...
 * bar: >= 3 zero-initialised words (zeroed again by every launch); hbar: FRTM_HBAR_WORDS words or NULL (flat barrier); stats (may be NULL):
 * [2] += 1 if the launch timed out (nothing is written back then), [3] += 1 if it committed.
 * ------------------------------------------------------------------------------------------ */
int frtm_joint_persistent_plan(int N, int Cin, int c, int h, int w, int* out4);
size_t frtm_joint_persistent_scratch(int N, int Cin, int c, int h, int w);
int frtm_joint_run_persistent(const float* X, const float* Z, const float* Bm, const float* cm, const float* sw, int N, int Cin, int c, int h, int w,
                              const float* w1T, float* w1, float* w2, float* vec, float* state, float* scratch, unsigned* bar, unsigned* hbar,
                              int iters, int has_p, int apply_dff, int fletcher_reeves, int standard_alpha, float dff, float lam1, float lam2,
                              float invM1, float invM2, float step, unsigned* stats, int debug_abort, frtm_stream_t stream);
/* y += a * x */
int frtm_vec_axpy(float* y, float a, const float* x, int n, frtm_stream_t stream);
/* out[c*rows + r] = in[r*cols + c]  (small 2-D transpose, rows x cols -> cols x rows) */
int frtm_transpose2d(const float* in, int rows, int cols, float* out, frtm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * fp32 MFMA implicit-GEMM convolution  (every conv of the ResNet trunk, feature_extractor.py:50-65;
 * the 1x1 projection, discriminator.py:81,203; the init-problem GEMMs)
 *   out[img, m, oy, ox] = epilogue( sum_{ci,kh,kw} wT[(ci,kh,kw), m] * in[img, ci, oy*s-pad+kh, ox*s-pad+kw] )
 *   epilogue: (* scale[m] + shift[m])?  (+ residual)?  relu?
 * wT: weights pre-transposed and zero padded to [Kp][Mp], Kp = K rounded up to 32 (K = Cin*kh*kw), Mp = Cout rounded
 *     up to 32 (see frtm_conv_pack_weights; FRTM_CONV_PACKED_ELEMS gives the element count).
 * ktab: int32[K*3] = {ci, kh, kw} built by frtm_conv_pack_weights; may be NULL for 1x1 convs.
 * out_transposed: write out[img, pix, m] instead of out[img, m, pix].
 * splitk: 0 = auto, 1 = none, >1: partial sums go through `workspace` (splitk*Cout*B*Ho*Wo floats; the factor is clamped
 *         to desc.ws_elems and to FRTM_CONV_MAX_SPLITK) and a second kernel applies the epilogue.
 * The init-problem weight gradient g1[c,ci] = sum_{img,pix} D[img,pix,c] * X[img,pix,ci] is the same
 * call with B=1, Cin = n_img*h*w, "pixels" = ci, wT = D (pixel-major) and in = X in NHWC.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  int B, Cin, Hin, Win, Cout, ksize, stride, pad;
  int relu, out_transposed;
  int splitk;              /* 0 = auto */
  int tile;                /* 0 = auto, else FRTM_TILE_* */
  int w_layout;            /* FRTM_WLAYOUT_GEMM (0) or FRTM_WLAYOUT_HALO3X3 (3x3, stride 1 or 2, pad 1 only), ... FRTM_WLAYOUT_BF16X3, FRTM_WLAYOUT_BF16X1 (below) */
  int ws_elems;            /* capacity of `workspace` in floats (0 = no workspace: split-K is disabled); split-K is clamped to it.
                              One workspace must not be used by convolutions that may run concurrently (one per stream). */
  int w_pitch;             /* 0: wT is the padded [Kp][Mp] image of frtm_conv_pack_weights;
                              >0: wT is a plain [K][w_pitch] matrix (w_pitch >= Cout, multiple of 4, 16-byte aligned) */
} frtm_conv_desc;
#define FRTM_CONV_MAX_SPLITK 32
/* Packed weight layouts.  GEMM: rows k = (ci,kh,kw), zero padded to [Kp][Mp].  HALO3X3: rows ordered
 * [ci/8][tap][ci%8] (72 rows per 8 input channels) for the halo-tile 3x3 kernel, which stages the raw
 * (TH+2)x(TW+2) input patch once per 8 channels instead of the 9x redundant im2col image. */
#define FRTM_WLAYOUT_GEMM 0
#define FRTM_WLAYOUT_HALO3X3 1
/* WINO3X3: Winograd F(2x2,3x3) transformed weights G g G^T, [ci/8][16 components][ci%8][Mp] (3x3, stride 1, pad 1 only;
 * no split-K: meant for launches with enough output blocks, the caller keeps the HALO3X3 image for the small ones). */
#define FRTM_WLAYOUT_WINO3X3 2
#define FRTM_CONV_WINO_ELEMS(Cout, Cin) ((((Cin) + 7) / 8 * 128) * (((Cout) + 31) / 32 * 32))
/* Winograd F(4x4,3x3) in three launches (conv_wino4.hip): input transform -> 36 batched [Cout x Cin] x [Cin x tiles] products (one
   launch of the fp32 MFMA GEMM kernel) -> output transform + epilogue.  frtm_conv2d then needs a workspace of
   FRTM_CONV_WINO4_WS_ELEMS floats; `tile` selects the GEMM tile (0 = auto).  3x3, stride 1, pad 1, NCHW only. */
#define FRTM_WLAYOUT_WINO4 3
#define FRTM_CONV_WINO4_ELEMS(Cout, Cin) (36 * (((Cin) + 31) / 32 * 32) * (((Cout) + 31) / 32 * 32))
#define FRTM_CONV_WINO4_TILES(B, H, W) ((((B) * (((H) + 3) / 4) * (((W) + 3) / 4)) + 63) / 64 * 64)
#define FRTM_CONV_WINO4_WS_ELEMS(B, Cin, Cout, H, W) ((size_t)36 * ((Cin) + (Cout)) * FRTM_CONV_WINO4_TILES(B, H, W))
/* ... and F(6x6,3x3) (points 0, +-1, +-2, +-1/2, inf; 64 products per 6x6 outputs = 1.78 multiplications per output; fp32 error of the
   same order as F(4x4): 2e-5 of the output range at 256 channels).  Fewer products AND smaller transformed tensors than F(4x4)
   whenever the map divides well into 6x6 tiles (30x54: no edge waste). */
#define FRTM_WLAYOUT_WINO6 4
#define FRTM_CONV_WINO6_ELEMS(Cout, Cin) (64 * (((Cin) + 31) / 32 * 32) * (((Cout) + 31) / 32 * 32))
#define FRTM_CONV_WINO6_TILES(B, H, W) ((((B) * (((H) + 5) / 6) * (((W) + 5) / 6)) + 63) / 64 * 64)
#define FRTM_CONV_WINO6_WS_ELEMS(B, Cin, Cout, H, W) ((size_t)64 * ((Cin) + (Cout)) * FRTM_CONV_WINO6_TILES(B, H, W))
/* bf16x3 (opt-in precision mode, csrc/conv_bf16x3.hip): 1x1, stride 1, pad 0, NCHW output, w_pitch 0, Cin % 16 == 0, tile 0, splitk 0 or 1;
   any Cout and H*W.  Weights and activations are split into three bf16 pieces (v = hi + mid + lo) and each product is formed from six piece
   products (hi.hi, hi.mid, mid.hi, hi.lo, mid.mid, lo.hi) on bf16 MFMAs with fp32 accumulation.  NOT bitwise an fmaf chain: against an fp64 product,
   on the trunk's 1x1 shapes at 1 and 8 frames, its max error is 0.78-1.40x and its rms error 0.93-1.28x those of the fp32 kernels
   (profiles/bf16x3_trunk_time.txt).  A NaN input stays a NaN; an Inf input gives NaN.
   Deterministic: bit-identical from launch to launch and for any grid.  The image is three bf16 planes [3][Cin/8][Mp][8], Mp = Cout rounded up
   to 128, stored in a float buffer of FRTM_CONV_BF16X3_ELEMS floats (16-byte aligned).  Other descriptors return FRTM_ERR_ARG. */
#define FRTM_WLAYOUT_BF16X3 5
#define FRTM_CONV_BF16X3_ELEMS(Cout, Cin) ((size_t)3 * (((Cin) + 15) / 16 * 16) * (((Cout) + 127) / 128 * 128) / 2)
/* bf16x1 (opt-in precision mode, csrc/conv_bf16x1.hip): 1x1, stride 1, pad 0, NCHW output, w_pitch 0, Cin % 16 == 0, splitk 0 or 1; any Cout and H*W.
   ONE bf16 piece per operand: out = epilogue(sum_k bf16(W) * bf16(X)), operands rounded to nearest even, products on bf16 MFMAs, fp32 accumulation
   and fp32 epilogue.  NOT fp32-level arithmetic: element-wise |out - exact| <= (2^-7 + 2^-16 + K 2^-22) (|W|.|X|).  NaN stays NaN, Inf stays Inf, |v|
   above the largest finite bf16 rounds to Inf; denormal operands are whatever the MFMA does with them.  Deterministic, and independent of the tile
   form and the grid (every output element is one fixed sequence of MFMAs).  `tile`: 0 = automatic (the large form for Cin >= 1024 when it has a tile per
   CU, else the small one), or FRTM_BF16X1_TILE_128x64 (1), FRTM_BF16X1_TILE_64x64 (2): Cout x pixels.  The image is one bf16 plane [Cin/8][Mp][8], Mp = Cout rounded up to 128, in a float
   buffer of FRTM_CONV_BF16X1_ELEMS floats (16-byte aligned).  Other descriptors return FRTM_ERR_ARG. */
#define FRTM_WLAYOUT_BF16X1 6
#define FRTM_CONV_BF16X1_ELEMS(Cout, Cin) ((size_t)(((Cin) + 15) / 16 * 16) * (((Cout) + 127) / 128 * 128) / 2)
#define FRTM_BF16X1_TILE_128x64 1
#define FRTM_BF16X1_TILE_64x64 2
/* bf16x1 for 3x3 convs (opt-in refiner precision mode, csrc/conv3x3_bf16x1.hip): 3x3, stride 1, pad 1 (zeros), NCHW output, w_pitch 0, splitk 0 or 1;
   any Cin, Cout, B, H, W.  The arithmetic and semantics of FRTM_WLAYOUT_BF16X1 in the direct form: out = epilogue(sum bf16(W) * bf16(X)), operands
   rounded once to nearest even, bf16 MFMAs, fp32 accumulation and epilogue; element-wise |out - exact| <= (2^-7 + 2^-16 + K 2^-22) |scale| (|W| conv |X|)
   with K = 9 Cin, plus the epilogue's fp32 rounding.  NaN stays NaN, Inf stays Inf; padding is zeros on both operands.  Deterministic, and independent of
   the tile form and the grid.  `tile`: 0 = automatic (the form with fewer padded rows), or FRTM_BF16X1_3X3_TILE_64 (1), FRTM_BF16X1_3X3_TILE_96 (2): output
   channels per workgroup, on 8 x 32 pixels.  The image is bf16 [Cin/16][tap][2][Mp][8], Mp = Cout rounded up to 32, in a float buffer of
   FRTM_CONV_BF16X1_3X3_ELEMS floats (16-byte aligned).  Other descriptors return FRTM_ERR_ARG.  FRTM_WLAYOUT_BF16X1 (6) keeps refusing 3x3 kernels. */
#define FRTM_WLAYOUT_BF16X1_3X3 7
#define FRTM_CONV_BF16X1_3X3_ELEMS(Cout, Cin) ((size_t)9 * (((Cin) + 15) / 16 * 16) * (((Cout) + 31) / 32 * 32) / 2)
#define FRTM_BF16X1_3X3_TILE_64 1
#define FRTM_BF16X1_3X3_TILE_96 2
/* The same for the 3x3 STRIDE-2 convs (opt-in bf16x1_3x3 trunk mode, csrc/conv3x3s2_bf16x1.hip): 3x3, stride 2, pad 1 (zeros), NCHW output, w_pitch 0,
   splitk 0 or 1; any Cin, Cout, B, H, W; Ho = (Hin - 1) / 2 + 1, Wo likewise.  Arithmetic, semantics, error bound, `tile` values and the weight image are
   those of FRTM_WLAYOUT_BF16X1_3X3: frtm_conv_pack_weights writes the SAME FRTM_CONV_BF16X1_3X3_ELEMS floats under either layout number.  Other
   descriptors (stride 1 among them) return FRTM_ERR_ARG; FRTM_WLAYOUT_BF16X1_3X3 (7) keeps refusing stride 2. */
#define FRTM_WLAYOUT_BF16X1_3X3_S2 8
#define FRTM_WINO_MIN_BLOCKS 512   /* 8x8 output blocks x 32-channel tiles below which callers prefer HALO3X3 + split-K */
#define FRTM_CONV_PACKED_ELEMS(Cout, Cin, k) \
  (((((Cin) * (k) * (k) + 31) / 32 * 32) > (((Cin) + 7) / 8 * 72) ? (((Cin) * (k) * (k) + 31) / 32 * 32) : (((Cin) + 7) / 8 * 72)) * (((Cout) + 31) / 32 * 32))
#define FRTM_TILE_64x64 1
#define FRTM_TILE_32x64 2
#define FRTM_TILE_128x64 3
#define FRTM_TILE_64x64_8W 4     /* 64x64 tile, 8 waves (two per SIMD) */
/* 5, 6: the 64-deep-chunk tiles of rounds 1-5 (an operand array in scratch memory, in no profile): removed in round 6 */
#define FRTM_TILE_64x128_8W 7
#define FRTM_TILE_128x128_8W 8   /* large-N regime: 32 FLOP per staged byte instead of 10.7 (32x64) */
#define FRTM_TILE_128x128_16W 9
#define FRTM_TILE_80x64 10       /* halo (3x3) kernel only: 65..80 output channels in one M tile */
/* 1x1 / stride-1 convs on v_mfma_f32_32x32x2_f32 (csrc/conv_gemm32.hip; NCHW output, H*W % 4 == 0, no split-K): Cout x pixel tile */
#define FRTM_TILE_G32_64x64 23   /* 4 waves of 32x32 (the only G32 tile left in round 5: the planner's choice for two layer3 GEMMs of the first-frame pass) */
int frtm_conv_pack_weights(const float* w_oihw, int Cout, int Cin, int ksize, int layout,
                           float* wT, int* ktab, frtm_stream_t stream);
int frtm_conv2d(const frtm_conv_desc* desc_host, const float* in, const float* wT, const int* ktab,
                const float* scale, const float* shift, const float* residual, float* out,
                float* workspace, frtm_stream_t stream);
/* Activation formats of frtm_conv2d_act (the opt-in bf16x1_act trunk mode, csrc/conv_bf16act.hip).
   FRTM_ACT_FP32 (0): dense NCHW fp32, what every other entry point reads and writes.
   FRTM_ACT_BF16 (1): bf16, channel-blocked by 8; needs C % 8 == 0 and a 16-byte aligned base.  Element (img, c, p) of a (B, C, H, W) tensor lies at
   bf16 index ((img * C/8 + c/8) * H*W + p) * 8 + c%8: every 8-channel slice of a pixel is 16 contiguous, 16-byte aligned bytes -- the [k/8][n][8]
   slot form in which the three bf16x1 kernels stage activations in LDS.  B*C*H*W*2 bytes.  Values are rounded on store to nearest even, the
   conversion the bf16x1 kernels apply to an fp32 input on load; NaN stays NaN and Inf stays Inf. */
#define FRTM_ACT_FP32 0
#define FRTM_ACT_BF16 1
/* frtm_conv2d with the input, the residual and the output each in its own format (in / residual / out point at fp32 or bf16 data accordingly; the
   residual's format is ignored when residual is NULL).  All three FRTM_ACT_FP32: frtm_conv2d itself.  Otherwise w_layout must be FRTM_WLAYOUT_BF16X1,
   _BF16X1_3X3 or _BF16X1_3X3_S2 with that layout's geometry, tile values and image; no out_transposed, no split-K, no w_pitch; Cin % 8 == 0 for a bf16
   input, Cout % 8 == 0 for a bf16 residual or output; bf16 tensors 16-byte aligned.  Anything else is FRTM_ERR_ARG and launches nothing.  The result is
   a bit-exact function of the fp32-format result of the same layout: a bf16 input changes nothing (the kernel rounds an fp32 input to bf16 anyway), a
   bf16 residual acts as its fp32 widening, a bf16 output is the fp32 output rounded to nearest even.  Workspace and ktab are not used by these forms. */
int frtm_conv2d_act(const frtm_conv_desc* desc_host, const void* in, const float* wT, const int* ktab,
                    const float* scale, const float* shift, const void* residual, void* out,
                    float* workspace, int in_fmt, int res_fmt, int out_fmt, frtm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Backbone: torchvision-topology ResNet trunk (model/feature_extractor.py:9-68), weights resident.
 * arch: 18, 34, 50, 101.  Parameters are uploaded per conv in forward order with their eval-mode
 * BatchNorm folded to (scale, shift).  forward() takes the uint8 image batch and writes the
 * requested taps (NULL = not wanted) as dense NCHW fp32.
 * ------------------------------------------------------------------------------------------ */
int frtm_backbone_create(int arch, frtm_backbone_t** out_host);
int frtm_backbone_destroy(frtm_backbone_t* bb);
int frtm_backbone_num_convs(const frtm_backbone_t* bb);
/* Shape of conv #idx in forward order: out6 = {Cout, Cin, ksize, stride, pad, has_residual_input} */
int frtm_backbone_conv_info(const frtm_backbone_t* bb, int idx, int* out6_host);
/* The form conv #idx takes for B images of Hin x Win input (under its own padding: ask the stem at the frame size) with the handle's modes and
 * plan as they are now: out3 = {FRTM_WLAYOUT_* of the launch, FRTM_TILE_* or 0, slot of frtm_backbone_last_flops_form}.  The decision of the
 * forward pass itself (csrc/trunk_route.h: choose_route) for a conv whose weights are loaded; needs neither weights nor a device. */
int frtm_backbone_conv_route(const frtm_backbone_t* bb, int idx, int B, int Hin, int Win, int* out3_host);
/* Per-conv launch plan override (0 = the planner's choice): `tile` = FRTM_TILE_* of the GEMM launch of whichever path the conv takes (the
 * direct 1x1 / gather conv, the batched products of the three-launch Winograd forms) or the output block 1..3 of the fused F(2x2,3x3)
 * kernel; `splitk` as in frtm_conv_desc.  Used by tools/trunk_tile_scan.py to scan tiles IN the trunk (concurrent lanes change the
 * ranking of the isolated scan) and by the planner's committed table.  Invalidates captured graphs (generation bump). */
int frtm_backbone_set_conv_plan(frtm_backbone_t* bb, int idx, int tile, int splitk);
int frtm_backbone_set_conv(frtm_backbone_t* bb, int idx, const float* w_oihw, const float* bn_scale,
                           const float* bn_shift, frtm_stream_t stream);
int frtm_backbone_forward(frtm_backbone_t* bb, const unsigned char* image_u8, int B, int H, int W,
                          const float* norm_scale3, const float* norm_bias3,
                          float* layer1, float* layer2, float* layer3, float* layer4, float* layer5,
                          int stop_after_layer, frtm_stream_t stream);
/* The same pass on lane set `lane_set` (0 or 1).  The two sets own separate activation arenas, scratch and internal streams, so ONE pass per
 * set may be in flight at a time: the first tracking pass of a sequence (set 0, enqueued before Tracker.initialize, reference
 * tracker.py:165-191) next to initialize()'s pass over the augmented first-frame stacks (set 1, feature_extractor.py:40-68 called from
 * tracker.py:186).  Results do not depend on the set. */
int frtm_backbone_forward_at(frtm_backbone_t* bb, int lane_set, const unsigned char* image_u8, int B, int H, int W, const float* norm_scale3,
                             const float* norm_bias3, float* layer1, float* layer2, float* layer3, float* layer4, float* layer5,
                             int stop_after_layer, frtm_stream_t stream);
/* hipStream_t of lane `lane` of the trunk (1 .. 2 * lanes - 1: the lanes of set 1 follow those of set 0); NULL for lane 0, which runs on
 * the caller's stream.  For the caller's stream placement (model/tracker.py: the first tracking pass of a sequence must not share a
 * hardware queue with the stream that runs Tracker.initialize, reference tracker.py:165-191). */
void* frtm_backbone_lane_stream(frtm_backbone_t* bb, int lane);
/* One wave that occupies `stream` for `microseconds` (0..100000): the probe with which the tracker finds out whether two streams share a
 * hardware queue (the runtime maps streams onto GPU_MAX_HW_QUEUES queues; streams of one queue run in order). */
int frtm_spin(int microseconds, frtm_stream_t stream);
/* One wave that reads both clocks for `microseconds` (1..100000): out2 (device, two 64-bit words) = {shader-clock cycles (s_memtime), ticks of the
 * constant 100 MHz counter}.  On a side stream next to a kernel sequence: the clock the shader holds under that load (bench.py: roofline.dominant_kernel). */
int frtm_clock_probe(int microseconds, unsigned long long* out2, frtm_stream_t stream);
/* HOST-side hole fill of the reference's first-frame augmentation: cv2.inpaint(image, hole, inpaintRadius = radius, cv2.INPAINT_TELEA)
 * (reference model/augmenter.py:317-324; the reference runs it on the CPU through OpenCV, once per object).  Restated from the published
 * fast-marching algorithm (csrc/telea_host.hip); every pointer is HOST memory, no GPU involved.  image / out: C planes of H x W uint8 (C <= 4),
 * hole: H x W, nonzero = pixel to fill.  The product's default first-frame fill (ImageAugmenter(fill='telea')); frtm_pull_push_fill is the
 * device-side alternative (fill='pull_push'). */
int frtm_telea_inpaint_u8(const unsigned char* image_chw, const unsigned char* hole_hw, int C, int H, int W, int radius, unsigned char* out_chw);
/* Launches of frtm_conv2d (this process) that took the PERSISTENT form of the 64x64 / 8-wave GEMM kernel (csrc/conv_igemm.hip: k_conv_igemm_p, round 6):
 * stride-1 1x1 convs with Cout % 64 == 0, Cin % 64 == 0, H*W % 4 == 0 and at least 1.5 tiles per resident workgroup.  FRTM_NO_PERSIST_GEMM=1 switches
 * the form off (A/B; results are bit-identical either way). */
long frtm_conv_persistent_launches(void);
/* The kernels that the last frtm_conv2d or frtm_conv_pack_weights call OF THE CALLING THREAD launched, space-separated in launch order, each named as its
 * demangled symbol without spaces and argument list: "k_conv3x3_halo<64,2,2,16,2> k_splitk_epilogue", "k_conv_igemm_p", "k_wino4_input
 * k_conv_igemm<64,64,2,4,1,32> k_wino4_output", ...  Empty after a call that failed before launching.  Host-side bookkeeping for the tests that
 * must know which kernel form a shape reached (tests/test_conv_forms_gpu.py); the pointer stays valid until the thread's next such call. */
const char* frtm_conv_last_kernels(void);
/* Launches of frtm_conv2d (this process) that took the bf16x3 form (FRTM_WLAYOUT_BF16X3, csrc/conv_bf16x3.hip). */
long frtm_conv_bf16x3_launches(void);
/* ... and that took the bf16x1 form (FRTM_WLAYOUT_BF16X1, csrc/conv_bf16x1.hip).  The two counters are disjoint. */
long frtm_conv_bf16x1_launches(void);
/* ... and that took the bf16x1 3x3 form (FRTM_WLAYOUT_BF16X1_3X3, csrc/conv3x3_bf16x1.hip): a counter of its own, the 1x1 counter does not move. */
long frtm_conv_bf16x1_3x3_launches(void);
/* ... and that took the bf16x1 3x3 stride-2 form (FRTM_WLAYOUT_BF16X1_3X3_S2, csrc/conv3x3s2_bf16x1.hip): its own counter again, the layout-7 one does not move. */
long frtm_conv_bf16x1_3x3s2_launches(void);
/* Launches of frtm_conv2d_act (this process) with at least one bf16 operand (csrc/conv_bf16act.hip).  Such a launch ALSO counts in the counter of its
 * layout above; an all-fp32 frtm_conv2d_act call is a frtm_conv2d call and does not count here. */
long frtm_conv_bf16act_launches(void);
/* Host-side check of the multiplication the conv kernels use instead of integer divisions in their index arithmetic (csrc/conv_common.h: FastDiv,
 * q = (mulhi(n, m) + n) >> s with m, s prepared per divisor): returns n / d as that formula computes it, for 0 <= n < 2^31, d >= 1.
 * No GPU involved; tests/test_cpu_host.py sweeps it against Python's integer division. */
unsigned frtm_fastdiv_check(unsigned n, unsigned d);
/* FLOPs (2*MAC over all convs) of the last forward() call. */
double frtm_backbone_last_flops(const frtm_backbone_t* bb);
/* The same with the launches that ran as Winograd F(2x2,3x3) counted at the multiplications they execute (16 / 36 of the direct form). */
double frtm_backbone_last_flops_executed(const frtm_backbone_t* bb);
/* algorithmic FLOPs of the last forward by kernel form: 0 = direct kernels, 1 = Winograd F(2x2,3x3), 2 = F(4x4,3x3), 3 = F(6x6,3x3) */
double frtm_backbone_last_flops_form(const frtm_backbone_t* bb, int form);
/* Number of convolutions (k_conv_igemm launches) of the last forward() call. */
int frtm_backbone_last_conv_launches(const frtm_backbone_t* bb);
/* Concurrency of forward(): a batch of B frames is split into min(lanes, B) sub-batches that run on the caller's stream
 * (lane 0) and on internal streams (lanes 1..), forked from / joined back to the caller's stream with events, so that the
 * call still behaves as one in-order operation on `stream`.  Frames are independent (feature_extractor.py:40-68), results
 * do not depend on the lane count.  lanes = 1 (default): everything on the caller's stream.  1 <= lanes <= 8. */
int frtm_backbone_set_lanes(frtm_backbone_t* bb, int lanes);
/* forward() allocates its activation arenas / split-K workspaces on first use and grows them (hipFree + hipMalloc, which
 * synchronises) when a larger batch or frame size arrives.  The counter returned here is bumped by every such
 * (re)allocation: a caller that captured forward() into a hipGraph must re-capture when it has changed, and must run a
 * shape once eagerly before capturing it (allocation is not allowed during stream capture). */
int frtm_backbone_generation(const frtm_backbone_t* bb);
/* The trunk's 3x3 stride-1 convs run as Winograd F(2x2,3x3) when a launch has >= FRTM_WINO_MIN_BLOCKS output blocks
 * (default on; results differ from the direct kernels by fp32 rounding only). */
int frtm_backbone_set_winograd(frtm_backbone_t* bb, int enable);
/* Three-launch Winograd (FRTM_WLAYOUT_WINO4 / WINO6) for the eligible 3x3 convs of a Winograd-enabled trunk: 0 = off, 1 = F(4x4,3x3)
   only, 2 (default) = F(4x4,3x3) or F(6x6,3x3), whichever needs fewer products for the map at hand. */
int frtm_backbone_set_winograd4(frtm_backbone_t* bb, int enable);
/* Trunk precision: 0 = fp32 (default), 1 = bf16x3 -- the stride-1 1x1 convs that the router picks run as FRTM_WLAYOUT_BF16X3,
 * in both lane sets and every lane; a per-conv plan (frtm_backbone_set_conv_plan) keeps its conv on the fp32 path.  The split weight images are
 * packed when mode 1 is first set (and again by a later frtm_backbone_set_conv); mode 0 allocates nothing.  Bumps the generation. */
int frtm_backbone_set_precision(frtm_backbone_t* bb, int mode);
/* The same switch by the number of bf16 pieces per operand: 0 = fp32, 3 = bf16x3 (identical to frtm_backbone_set_precision(bb, 1)), 1 = bf16x1 --
 * the stride-1 1x1 convs that the bf16x1 router picks (csrc/trunk_route.h: kTrunkRules, profiles/bf16x1_trunk_time.txt) run as FRTM_WLAYOUT_BF16X1.
 * Anything else (2 included) is FRTM_ERR_ARG and leaves the mode as it was.  The two bf16 modes are exclusive: a bf16x1 trunk never launches the
 * bf16x3 kernel.  Images are packed when the mode is first set (and again by a later frtm_backbone_set_conv); bumps the generation when the mode
 * changes.  A per-conv plan keeps its conv on the fp32 path.  Environment FRTM_BF16X1_MIN_COLS=n (read at frtm_backbone_create; for tests and
 * measurements on small frames): every eligible conv of a bf16x1 trunk is routed from n columns per launch on, instead of the measured table. */
int frtm_backbone_set_bf16_pieces(frtm_backbone_t* bb, int pieces);
/* The 3x3 convs of a bf16x1 trunk on bf16 MFMAs as well (the bf16x1_3x3 trunk mode): on = 1 / 0; anything else is FRTM_ERR_ARG and leaves the state as
 * it was.  The flag is stored independently of the pieces mode and takes effect only while that mode is 1 (bf16x1): then a 3x3 pad-1 conv of stride 1
 * runs as FRTM_WLAYOUT_BF16X1_3X3 and one of stride 2 as FRTM_WLAYOUT_BF16X1_3X3_S2, where the 3x3 router picks it (csrc/trunk_route.h: kTrunkRules,
 * profiles/bf16x1_trunk3x3_time.txt; under FRTM_BF16X1_MIN_COLS=n every such conv from n columns per launch on) and the conv has no per-conv plan.  The
 * stem and the 1x1 convs are handled as without the flag.  Images are packed when the flag first turns on (and again by a later
 * frtm_backbone_set_conv): for every 3x3 conv of ResNet-101 about 43 MB of device memory.  Bumps the generation when the flag's value changes. */
int frtm_backbone_set_bf16x1_3x3(frtm_backbone_t* bb, int on);
/* bf16 storage of the activations that only bf16 kernels touch (the bf16x1_act trunk mode): on = 1 / 0; anything else is FRTM_ERR_ARG and leaves the
 * state as it was.  Stored whatever the other switches are; takes effect only while the pieces mode is 1 AND the 3x3 flag is on.  Then a tensor of
 * the block walk (a block's t1 / t2, a downsample output, a block output that does not end a stage) is held as FRTM_ACT_BF16 exactly when its
 * channel count is a multiple of 8, the conv that writes it is routed to layout 6, 7 or 8 at that launch, and so is EVERY conv that reads it, as
 * input or as residual (csrc/trunk_route.h: act_plan).  The normalised image, the stem and pool outputs, every stage output (every tap, wanted or
 * not) and anything an fp32 form touches stay fp32, so the fp32 kernels never meet a bf16 tensor and the taps stay dense NCHW fp32.  Against
 * bf16x1_3x3 the only new rounding is the value a residual operand carries.  Needs no new weight image; the arenas are unchanged (a bf16 tensor
 * uses half of its buffer).  Bumps the generation when the flag's value changes. */
int frtm_backbone_set_bf16_act(frtm_backbone_t* bb, int on);
/* The formats of one pass of B frames per lane at H x W with the handle's modes as they are now: out3_per_conv[3 * i .. 3 * i + 2] = the
 * {input, residual, output} FRTM_ACT_* of conv #i (forward order, as frtm_backbone_conv_info).  `capacity`: convs the buffer holds, at least
 * frtm_backbone_num_convs.  All zero unless the bf16x1_act mode is in effect.  The decision of the forward pass itself; needs neither weights nor a
 * device. */
int frtm_backbone_act_plan(const frtm_backbone_t* bb, int B, int H, int W, int* out3_per_conv, int capacity);

/* ------------------------------------------------------------------------------------------
 * Tracker.track mask merge (model/tracker.py:214-221), in place on masks (n_obj+1, H*W).
 * ------------------------------------------------------------------------------------------ */
int frtm_merge_masks(float* masks, int n_plus_1, int HW, frtm_stream_t stream);
/* The same for `frames` consecutive (n_obj+1, H*W) stacks (a tracking window), one launch. */
int frtm_merge_masks_frames(float* masks, int frames, int n_plus_1, int HW, frtm_stream_t stream);
/* The tail of Tracker.track for a window of `frames` frames in one pass (reference model/tracker.py:200-221, label decoding of
 * run_sequence :143-150, pixel counts for discriminator.py:214): logits (frames, n_obj, HW) of the refiner -> sigmoid -> merge ->
 * masks (frames, n_obj + 1, HW); optional labels (frames, HW) uint8 = lut[decoded class] (lut: n_obj + 1 bytes on the device;
 * single_object_decode != 0: the one-object rule masks[1] > 0.5) and counts (frames, n_obj + 1) int32 = pixels above thr per plane.
 * At most 15 objects (more: frtm_merge_masks_frames + frtm_count_above). */
int frtm_track_merge(const float* logits, int frames, int n_obj, int HW, float* masks, unsigned char* labels, const unsigned char* lut,
                     int single_object_decode, int* counts, float thr, frtm_stream_t stream);
/* frtm_filter_scores with a pitch (floats) between the output maps of consecutive samples (>= h*w). */
int frtm_filter_scores_pitched(const float* X, const float* f, int N, int C, int h, int w, float* out, int out_pitch, int accumulate,
                               frtm_stream_t stream);
/* Grouped target-model scoring (csrc/target_apply_grouped.hip): for G (frame, target) pairs, what G calls of frtm_conv2d (1x1 projection)
 * + frtm_filter_scores on one frame each compute, in two launches.
 *   feats          base of a feature batch (F, Cin, h, w); frame_pitch floats between frames (>= Cin*h*w: the frames need not be dense)
 *   frame_of_pair  device int32[G]: the frame pair p reads; several pairs may name one frame (a pair naming none of the F frames is skipped:
 *                  its slices of cft and of scores are left untouched)
 *   w1T, w2        device tables of G pointers: projection in GEMM layout [Cin][c]; filter (1, c, 3, 3)
 *   cft            (G, c, h, w) dense: pair p's projected features;   scores (G, 1, h, w) dense, in pair order
 * Projection on fp32 MFMA, no split-K, no atomics: every element is one chain over K = Cin in ascending order; the 3x3 pass (zero
 * padding) has one fixed summation order.  A pair's result does not depend on G, its place in the tables or the other pairs.
 * Any h, w; c <= 128; Cin a multiple of 32; everything else fails with FRTM_ERR_ARG. */
int frtm_target_apply_grouped(const float* feats, size_t frame_pitch, int F, const int* frame_of_pair, const float* const* w1T,
                              const float* const* w2, int G, int Cin, int c, int h, int w, float* cft, float* scores, frtm_stream_t stream);
/* The tile form frtm_target_apply_grouped projects G pairs of c channels on an h x w map with: *fm = ceil(c / 32) in 1..4 (a tile holds
 * 32 * fm rows, all c channels), *fn = 2 (64-pixel tiles) when ceil(h*w / 64) * G >= 256, else 1 (32-pixel tiles).  Host only, no launch:
 * the launcher itself calls it, and so do the tests to know which of the eight compiled forms a shape runs.  FRTM_ERR_ARG outside
 * 1 <= G <= 65535, 1 <= c <= 128, 1 <= h*w <= 2^24. */
int frtm_target_apply_grouped_tiles(int G, int c, int h, int w, int* fm, int* fn);
/* count[k] = #pixels with masks[k] > 0.5   (the early-out test of discriminator.py:214), int32[n] */
int frtm_count_above(const float* masks, int n, int HW, float thr, int* count, frtm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Refinement network glue (model/seg_network.py:7-189); its convolutions go through frtm_conv2d / frtm_filter_scores.
 * ------------------------------------------------------------------------------------------ */
/* F.interpolate(..., 'bilinear', align_corners=False) of `planes` maps (lib/utils.py:33-35) */
int frtm_bilinear_resize(const float* in, int planes, int h, int w, float* out, int H, int W, frtm_stream_t stream);
/* TSE: out[s,c] = relu(base[s/group,c] + bias[c] + conv3x3(bilinear(scores[s]) , ws[c]))  (seg_network.py:16-21 with the
 * object-independent 64-channel part of transform[0] pre-computed in base (n/group,C,H,W): `group` consecutive samples = the
 * objects of one frame share a map); scores (n,1,h,w), out (n,C,H,W). */
int frtm_tse_inject(const float* base, const float* bias, const float* ws, const float* scores, int n, int group, int C,
                    int h, int w, int H, int W, float* out, frtm_stream_t stream);
/* CAB (seg_network.py:38-41): out = shallow * sigmoid(gate[s,c]) + bilinear(deeper[d,c], (hd,wd) -> (H,W)), d = s / deeper_group
 * when deeper_group > 0 (objects of a frame share the deeper map: the pooled vector of the deepest level), d = s when it is 0. */
int frtm_cab_combine(const float* shallow, const float* gate, const float* deeper, int n, int C, int hd, int wd, int deeper_group,
                     int H, int W, float* out, frtm_stream_t stream);
/* CAB gate (model/seg_network.py:34-37, before the sigmoid): gate (n,oc) = W2^T relu(W1^T cat(sp, dp) + b1) + b2.
 * sp: (n,oc) pooled shallower features; dp: pooled deeper features, row s / dp_group when dp_group > 0, row s when it is 0;
 * W1 (2oc,oc) and W2 (oc,oc): the two 1x1 conv weights transposed to [in][out]. */
int frtm_cab_gate(const float* sp, const float* dp, int dp_group, const float* W1, const float* b1, const float* W2, const float* b2,
                  int n, int oc, float* gate, frtm_stream_t stream);
/* The indexed twins (csrc/ragged_group.hip) for frames that carry different numbers of objects: the frame of sample s comes from a
 * device int32 table instead of s / group -- the frame_of_pair table of frtm_target_apply_grouped, so one table serves the scoring
 * and the refiner.  Per sample the arithmetic is that of the kernel named: with the table s / group the outputs are bit-identical, and
 * a sample's output does not depend on the rest of the launch.  A sample whose entry lies outside [0, F) (rows, entries) is skipped
 * and its output left untouched; nothing is read or written out of bounds whatever the table holds.  Size and grid limits as the twins.
 *   frtm_tse_inject_indexed    out[s] = relu(base[frame_of[s]] + bias + conv3x3(bilinear(scores[s]), ws)); base (F,C,H,W), frame_of int32[n]
 *   frtm_cab_gate_indexed      frtm_cab_gate with the deeper pooled row dp[row_of[s]]; dp (rows,oc), row_of int32[n]
 *   frtm_cab_combine_indexed   frtm_cab_combine with the deeper entry deeper[entry_of[s]]; deeper (entries,C,hd,wd), any hd, wd */
int frtm_tse_inject_indexed(const float* base, const float* bias, const float* ws, const float* scores, int n, const int* frame_of, int F,
                            int C, int h, int w, int H, int W, float* out, frtm_stream_t stream);
int frtm_cab_gate_indexed(const float* sp, const float* dp, const int* row_of, int rows, const float* W1, const float* b1, const float* W2,
                          const float* b2, int n, int oc, float* gate, frtm_stream_t stream);
int frtm_cab_combine_indexed(const float* shallow, const float* gate, const float* deeper, const int* entry_of, int entries, int n, int C,
                             int hd, int wd, int H, int W, float* out, frtm_stream_t stream);
/* frtm_track_merge for frames with different object counts, without the label decoding.  first: device int32[frames + 1], the exclusive
 * prefix sums of the per-frame counts n_f (first[0] = 0).  Frame f reads the logit planes first[f] .. first[f+1] - 1 of logits
 * (first[frames], HW) and writes its n_f + 1 mask planes, packed, from plane first[f] + f of masks (first[frames] + frames, HW) on;
 * counts (first[frames] + frames) int32, packed the same way, or NULL.  1 <= n_f <= 15; a frame whose entries break that, are negative
 * or pass first[frames] is skipped, its masks and counts left untouched.  On equal counts the result is frtm_track_merge's, bit for bit. */
int frtm_track_merge_ragged(const float* logits, int frames, const int* first, int HW, float* masks, int* counts, float thr,
                            frtm_stream_t stream);
/* PyrUpBicubic2d: 2x polyphase bicubic with replicate border (seg_network.py:75-126); out (planes,2h,2w) */
int frtm_pyrup2x(const float* in, int planes, int h, int w, float* out, frtm_stream_t stream);
/* Whether the fused tail takes a (h,w) -> (Ho,Wo) resize (1) or its LDS patch is too small for the ratio (0).  h, w: the size of the map
 * handed to the tail kernel; bicubic == 0: frtm_project_tail, else frtm_project_tail_bicubic.  Host only, no launch: the argument
 * checks of the two entry points call it, and so do their callers to choose between the fused and the unfused form. */
int frtm_project_tail_fits(int bicubic, int h, int w, int Ho, int Wo);
/* Tail of BackwardCompatibleUpsampler.forward (model/seg_network.py:117-119) in one kernel:
 *   out[n,0] = conv2(interpolate(up2(y[n]), (Ho,Wo), bilinear, align_corners=False)) + bias
 * y (n,C,h,w) is relu(conv1(up1(x))); up2 = PyrUpBicubic2d (2x), conv2 = 3x3, C -> 1, zero padding.  w3x3 (1,C,3,3), bias (1)
 * or NULL.  The resize ratio 2h/Ho, 2w/Wo must be within ~[0.5, 1.1] (the LDS patch of the fused kernel); otherwise the call
 * fails with FRTM_ERR_ARG and the caller composes frtm_pyrup2x + frtm_bilinear_resize + frtm_filter_scores. */
int frtm_project_tail(const float* y, int n, int C, int h, int w, const float* w3x3, const float* bias, int Ho, int Wo, float* out,
                      frtm_stream_t stream);
/* The channel sum of conv2 taken BEFORE the two resampling steps (they are linear and act per channel):
 *   out[n,t] = sum_c w3x3[c*9 + t] * y[n,c]      (t = 0..8: the nine taps; y (n,C,h*w), out (n,9,h*w))
 * frtm_project_tail(out, n, 9, h, w, one-hot weights (9,3,3): eye(9), bias, ..) then equals frtm_project_tail(y, n, C, h, w, w3x3, bias, ..)
 * up to summation order, with 9 instead of C maps resampled (model/seg_network.py:117-119). */
int frtm_tap_mix(const float* y, int n, int C, int hw, const float* w3x3, float* out, frtm_stream_t stream);
/* F.interpolate(..., (H,W), 'bicubic', align_corners=False) of `planes` maps (model/seg_network.py: Upsampler), any ratio up or down:
 * source coordinate (dst + 0.5) * in/out - 0.5 (no clamp at 0), taps floor - 1 .. floor + 2 clamped into the map, A = -0.75. */
int frtm_bicubic_resize(const float* in, int planes, int h, int w, float* out, int H, int W, frtm_stream_t stream);
/* Tail of Upsampler.forward (model/seg_network.py) in one kernel:
 *   out[n,0] = conv2(interpolate(y[n], (Ho,Wo), bicubic, align_corners=False)) + bias
 * y (n,C,h,w) is relu(conv1(2x bicubic(x))); conv2 = 3x3, C -> 1, zero padding.  w3x3 (1,C,3,3), bias (1) or NULL.  Takes the nine
 * tap maps of frtm_tap_mix with one-hot weights like frtm_project_tail.  The upscale Ho/h, Wo/w must be at least ~1.6 x ~1.9 (the LDS
 * patch of the fused kernel); otherwise the call fails with FRTM_ERR_ARG and the caller composes frtm_bicubic_resize + frtm_filter_scores. */
int frtm_project_tail_bicubic(const float* y, int n, int C, int h, int w, const float* w3x3, const float* bias, int Ho, int Wo, float* out,
                              frtm_stream_t stream);
/* adaptive_avg_pool2d(x, 1): out[plane] = mean(in[plane]) */
int frtm_plane_mean(const float* in, int planes, int HW, float* out, frtm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Refiner training (SegNetwork.forward_train, model/refiner_train.py): train-mode BatchNorm and the backward pass.
 * No atomics: every reduction runs in a fixed order, so repeated backward passes are bitwise identical.
 * ------------------------------------------------------------------------------------------ */
/* Weight gradient of a stride-1, pad-k/2 conv (k = 1 or 3): dw (Cout,Cin,k,k) = sum over (n,y,x) of dy (B,Cout,H,W) times the
 * shifted x (B,Cin,H,W); dbias (Cout) = sum of dy.  Either output may be NULL (not both).  fp32 MFMA over pixel chunks into
 * ws (>= frtm_conv_wgrad_ws_elems floats), then an fp64 fixed-order sum of the chunks. */
size_t frtm_conv_wgrad_ws_elems(int B, int Cout, int Cin, int k, int H, int W);
int frtm_conv_wgrad(const float* dy, const float* x, int B, int Cout, int Cin, int k, int H, int W, float* dw, float* dbias, float* ws,
                    size_t ws_elems, frtm_stream_t stream);
/* The same for k = 3 in bf16x1 arithmetic (csrc/conv_wgrad_bf16x1.hip; the opt-in SegNetwork.train_precision = 'bf16x1'): dy and x are each rounded
 * to bf16 once, to nearest even, the products run on v_mfma_f32_32x32x16_bf16, accumulation is fp32 in chains of at most 2048 pixels, and the
 * chains' slabs in ws (>= frtm_conv_wgrad_bf16x1_ws_elems floats) are summed in fp64 in a fixed order.  dbias is the ones column of the same
 * product: the sum of bf16(dy).  Up to 2^-7 of |dy| (x) |x| per element: NOT fp32-level arithmetic.  No atomics; the arguments as above. */
size_t frtm_conv_wgrad_bf16x1_ws_elems(int B, int Cout, int Cin, int H, int W);
int frtm_conv_wgrad_bf16x1(const float* dy, const float* x, int B, int Cout, int Cin, int H, int W, float* dw, float* dbias, float* ws,
                           size_t ws_elems, frtm_stream_t stream);
/* Launches of frtm_conv_wgrad_bf16x1 (this process), like frtm_conv_bf16x1_3x3_launches. */
long frtm_conv_wgrad_bf16x1_launches(void);
/* BatchNorm2d statistics of x (N,C,HW).  train = 1: batch mean and 1/sqrt(biased var + eps) -> mean, invstd; when rmean / rvar are
 * given, they are updated as nn.BatchNorm2d does with factor = momentum (or 1/num_batches_tracked for momentum=None; 0: no update),
 * unbiased variance.  part: >= 2*N*C doubles.  train = 0: mean = rmean, invstd = 1/sqrt(rvar + eps) (part unused). */
int frtm_bn_stats(const float* x, int N, int C, int HW, float eps, float factor, int train, float* rmean, float* rvar, float* mean,
                  float* invstd, double* part, frtm_stream_t stream);
/* out = relu((x - mean[c]) * invstd[c] * gamma[c] + beta[c]) */
int frtm_bn_apply_relu(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta, int N, int C, int HW,
                       float* out, frtm_stream_t stream);
/* Backward of frtm_bn_apply_relu: g = dy * (out > 0); train: dx = gamma*invstd/n * (n g - sum g - (xhat - sum xhat / n) sum g xhat) (in fp64, one
 * rounding; xhat is centred on the fp32 mean, its own mean is taken out so that sum dx vanishes), eval: dx = gamma*invstd*g; dgamma = sum g xhat,
 * dbeta = sum g (either may be NULL).  part: >= 3*N*C doubles. */
int frtm_bn_relu_backward(const float* dy, const float* out, const float* x, const float* mean, const float* invstd, const float* gamma,
                          int N, int C, int HW, int train, float* dx, float* dgamma, float* dbeta, double* part, frtm_stream_t stream);
/* dx = y > 0 ? dy : 0 for n elements (ReLU backward from the saved output; dx may alias dy) */
int frtm_relu_backward(const float* dy, const float* y, size_t n, float* dx, frtm_stream_t stream);
/* Transpose of frtm_pyrup2x: dout (planes,2h,2w) -> din (planes,h,w); tmp: planes*2h*w floats */
int frtm_pyrup2x_backward(const float* dout, int planes, int h, int w, float* din, float* tmp, frtm_stream_t stream);
/* Transpose of frtm_bilinear_resize (h,w) -> (H,W): dout (planes,H,W) -> din (planes,h,w); tmp: planes*H*w floats */
int frtm_bilinear_backward(const float* dout, int planes, int h, int w, int H, int W, float* din, float* tmp, frtm_stream_t stream);
/* CAB backward, per plane of dout / shallow (planes,HW): a = sum dout*shallow, b = sum dout */
int frtm_cab_backward_reduce(const float* dout, const float* shallow, int planes, int HW, float* a, float* b, frtm_stream_t stream);
/* Backward of frtm_cab_gate and the sigmoid: dg = a * sig'(gate); W1 (oc,2oc), W2 (oc,oc) in the conv layout [out][in]; sp, dp, gate, a
 * (n,oc).  Writes dW1, db1, dW2, db2 (each may be NULL), dsp and ddp (n,oc); badd (n,oc) or NULL is added to ddp. */
int frtm_cab_gate_backward(const float* sp, const float* dp, const float* gate, const float* a, const float* badd, const float* W1,
                           const float* b1, const float* W2, int n, int oc, float* dW1, float* db1, float* dW2, float* db2, float* dsp,
                           float* ddp, frtm_stream_t stream);
/* ds = dout * sigmoid(gate[plane]) + dsp[plane] / HW */
int frtm_cab_backward_shallow(const float* dout, const float* gate, const float* dsp, int planes, int HW, float* ds, frtm_stream_t stream);
/* x[plane] += v[plane] * scale */
int frtm_add_plane(float* x, const float* v, float scale, int planes, int HW, frtm_stream_t stream);
/* out (n,9,H,W): out[n,t,y,x] = dl[n,0,y-ky+1,x-kx+1], t = 3ky+kx, 0 outside (the input gradient of a 3x3 conv's nine taps) */
int frtm_shift9(const float* dl, int n, int H, int W, float* out, frtm_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Affine warp of C planes (replaces lib/_npp/nppig.cpp:48-104 = NVIDIA NPP nppiWarpAffine_*, called from
 * lib/image.py:53).  fwd6_host: HOST float[6], the forward 2x3 transform (source -> destination), as
 * cv2.warpAffine / NPP take it.  mode: 0 nearest, 1 bilinear, 2 bicubic.  Outside pixels become 0.
 * ------------------------------------------------------------------------------------------ */
int frtm_warp_affine(const float* src, int C, int Hs, int Ws, float* dst, int Hd, int Wd,
                     const float* fwd6_host, int mode, frtm_stream_t stream);
/* The uint8 entry point of the reference's extension (nppig.cpp:99-100, nppiWarpAffine_8u_C1R): uint8 planes in, uint8 planes out;
 * nearest copies, bilinear / bicubic round the float interpolant to nearest and saturate. */
int frtm_warp_affine_u8(const unsigned char* src, int C, int Hs, int Ws, unsigned char* dst, int Hd, int Wd, const float* fwd6_host,
                        int mode, frtm_stream_t stream);
/* n <= 32 nearest-neighbour warps of ONE mask plane (nonzero = set) in one launch: dst (n,Hd,Wd) uint8 {0,1}, count_dev int32[n] =
 * set pixels per warp.  fwd6_host: n forward 2x3 transforms (host memory).  The augmenter's candidate test (reference
 * model/augmenter.py:454-471 verify_frame looks at the candidates' label pixel counts only). */
int frtm_warp_mask_batch(const float* src, int Hs, int Ws, unsigned char* dst, int Hd, int Wd, const float* fwd6_host, int n,
                         int* count_dev, frtm_stream_t stream);

/* ---- round 4: the rest of the first-frame augmentation (reference model/augmenter.py:297-345,365-390,454-555) as device kernels ----
 * frtm_mask_stats: pixel count and bounding box of a mask plane (uint8 or float, set = > 0) into DEVICE int32[5]
 *   {count, max(x+1), max(W-x), max(y+1), max(H-y)} (x1 = [1]-1, x0 = W-[2], y1 = [3]-1, y0 = H-[4]); replaces the torch reductions +
 *   host read of the reference's bounding-box code (augmenter.py:285-295, np.where on the host). */
int frtm_mask_stats(const void* mask, int is_u8, int H, int W, int* out5_dev, frtm_stream_t stream);
/* The cut (augmenter.py:297-316): target4 = (image * mask, mask * 255) as float planes, mask_f = the {0,1} mask, label01_out (may be
 * NULL) = the binarised label, pyr0_4 = level 0 of the fill pyramid: image * (1 - hole) and the known plane 1 - hole, hole = the mask
 * dilated by one pixel. */
int frtm_aug_prepare(const unsigned char* image_u8, const unsigned char* label_u8, int H, int W, float* target4, float* pyr0_4,
                     float* mask_f, unsigned char* label01_out, frtm_stream_t stream);
/* Pull-push hole fill over the pyramid buffer (frtm_pull_push_elems(H, W) floats, level 0 from frtm_aug_prepare): the stand-in for
 * cv2.inpaint(..., INPAINT_TELEA) (augmenter.py:317-324; OpenCV is absent).  Afterwards the three colour planes
 * of level 0 hold the filled background, clamped to [0, 255] and floored. */
int frtm_pull_push_fill(float* pyr, size_t pyr_elems, int H, int W, frtm_stream_t stream);
size_t frtm_pull_push_elems(int H, int W);
/* get_transform (augmenter.py:230-283) for n candidate specs ON THE DEVICE, from the bounding box frtm_mask_stats left there.
 * spec10_dev: double[n][10] = {scale, scale relative to the target height (0/1), fliplr, rotation in degrees, skew x, skew y,
 * location x, location y (fractions of the image), min_size, limit_scale}.  Out: forward and inverse 2x3 as float32 [n][6]. */
int frtm_aug_transforms(const double* spec10_dev, int n, const int* stats5_dev, int H, int W, float* fwd6_dev, float* inv6_dev,
                        frtm_stream_t stream);
/* frtm_warp_mask_batch with the INVERSE matrices in device memory (n unbounded). */
int frtm_warp_mask_batch_dev(const float* src, int Hs, int Ws, unsigned char* dst, int Hd, int Wd, const float* inv6_dev, int n,
                             int* count_dev, frtm_stream_t stream);
/* n bicubic warps (a = -0.75, zero outside, result clamped to [0, 255]) of the same C float planes: dst [n][C][Hd][Wd]; matrix of
 * warp j = inv6_dev[index_dev ? index_dev[j] : j] (augmenter.py:365-379 warps target and background of each sample one by one). */
int frtm_warp_affine_batch(const float* src, int C, int Hs, int Ws, float* dst, int Hd, int Wd, const float* inv6_dev,
                           const int* index_dev, int n, frtm_stream_t stream);
/* The paste (augmenter.py:380-390) for n samples: alpha = wt4[j][3] / 255, image = wt4[j][:3] * alpha + canvas3[j] * (1 - alpha)
 * truncated to uint8; label j = candidate plane cand_labels[index_dev[j]]. */
int frtm_aug_blend(const float* wt4, const float* canvas3, int n, int H, int W, const unsigned char* cand_labels,
                   const int* index_dev, unsigned char* out_images, unsigned char* out_labels, frtm_stream_t stream);

/* n 32-bit words <- pattern (a runtime memset node): the zero / one fills of per-sequence state on the initialize() path
 * (reference: torch.zeros / fill_ in tracker.py:166, memory.py:33-48, optimizer.py:29-40). */
int frtm_fill32(void* dst, size_t n_words, unsigned pattern, frtm_stream_t stream);
/* mask = (labels == obj_id) as uint8 {0,1} and, if plane_f32 != NULL, as a float plane (reference tracker.py:170-172,188). */
int frtm_label_mask(const unsigned char* labels_u8, int obj_id, size_t n, unsigned char* mask_u8, float* plane_f32, frtm_stream_t stream);

/* dst[p,y,x] = sum_{i,j} G[i,j] * src[p, y+i-kh/2, x+j-kw/2], zero outside (the augmenter's blur, model/augmenter.py:330-345:
 * cv2.filter2D / F.conv2d(padding=k//2) semantics).  G: DEVICE float[kh*kw], odd kh, kw. */
int frtm_blur2d(const float* src, int planes, int H, int W, const float* G, int kh, int kw, float* dst, frtm_stream_t stream);
/* The same with G = the normalised Gaussian exp(-(qa x^2 + 2 qb x y + qc y^2)/2) on [-half, half]^2 (x along the row), formed
 * inside the kernel from the inverse covariance (qa qb; qb qc): the augmenter's motion blur with no host -> device upload. */
int frtm_blur_gauss2d(const float* src, int planes, int H, int W, int half, float qa, float qb, float qc, float* dst,
                      frtm_stream_t stream);

/* The DAVIS measures J and F (lib/davis.py: db_eval_iou, seg2bmap, db_eval_boundary) as exact integer counts (csrc/jf_eval.hip).
 * pred / truth: DEVICE label maps [T][H][W], label_bytes = 1 (uint8) or 4 (int32); ids: HOST array of K object ids; r: radius of the
 * matching disk {dy^2 + dx^2 <= r^2} in pixels, 1 ... 64.  counts: DEVICE int32 [T][K][6] = inter, union (of pred == id and
 * truth == id), n_fg, n_gt (boundary pixels of either), fg_match, gt_match (boundary pixels with a boundary pixel of the other map
 * inside the disk; zero outside the image).  ws: frtm_jf_workspace_bytes(T, H, W, K) bytes of device scratch (the boundary maps as
 * bit planes).  H * W < 2^31 and T * K * 2 <= 65535 per call (the caller splits longer sequences over frames). */
size_t frtm_jf_workspace_bytes(int T, int H, int W, int K);
int frtm_jf_counts(const void* pred, const void* truth, int label_bytes, int T, int H, int W, const int* ids, int K, int r, int* counts,
                   void* ws, size_t ws_bytes, frtm_stream_t stream);

/* The loss tail of a refiner training step in one pass (csrc/train_step.hip; model/train_loss.py): BCELoss(sigmoid(z), t) as a function
 * of real numbers.  logits: DEVICE z [N][1][H][W] fp32; target: DEVICE t of the same shape, target_bytes = 1 (uint8 {0,1}) or 4 (fp32
 * in [0,1], soft targets allowed).  Outputs, all DEVICE: loss[1] = mean of t * min(softplus(-z), 100) + (1 - t) * min(softplus(z), 100)
 * (fp32 terms, summed in fp64 in a fixed order: per-workgroup partials in ws, a second launch adds them, a wave per sample; no atomics);
 * dlogits (may be NULL: evaluation only) = (sigmoid(z) - t) / (N H W), the part of a term whose clamp at 100 binds contributing nothing;
 * inter[N] / uni[N] = int32 counts of (z > 0) & (t > 0.5) and (z > 0) | (t > 0.5) per sample (the inputs of mask_iou).
 * logits, dlogits and fp32 targets must be 16-byte aligned (uint8 targets 4-byte); ws: frtm_bce_logits_workspace_bytes(N, H, W) bytes,
 * 8-byte aligned.  N <= 65535. */
size_t frtm_bce_logits_workspace_bytes(int N, int H, int W);
int frtm_bce_logits(const float* logits, const void* target, int target_bytes, int N, int H, int W, float* dlogits, float* loss, int* inter,
                    int* uni, void* ws, size_t ws_bytes, frtm_stream_t stream);

/* x[i] *= scale[0] for n floats, scale a DEVICE scalar (the loss's incoming gradient applied to dlogits without a host read-back).
 * x 16-byte aligned. */
int frtm_scale_by(float* x, size_t n, const float* scale, frtm_stream_t stream);

/* torch.optim.Adam's update for one parameter group in one launch (csrc/train_step.hip; lib/fused_adam.py), per element in fp32:
 *   g += wd * p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  vmax = max(vmax, v)  [amsgrad];
 *   p -= (lr / bias_correction1) * m / (sqrt(vmax or v) / sqrt(bias_correction2) + eps).
 * tensors: DEVICE table, eight 64-bit words per tensor = pointers p, grad, exp_avg, exp_avg_sq, max_exp_avg_sq (ignored unless amsgrad),
 * element count, 1 if all five pointers are 16-byte aligned (else the tensor is walked element by element), 0.  chunks: DEVICE int32
 * pairs (tensor index, chunk index): chunk c of a tensor is its elements [c * E, min((c + 1) * E, count)), E = frtm_adam_chunk_elems();
 * every tensor needs ceil(count / E) chunks.  Pairs outside the table are skipped.  The scalars are launch arguments: a learning-rate
 * schedule changes no table. */
int frtm_adam_chunk_elems(void);
int frtm_adam_amsgrad(const void* tensors, int ntensors, const void* chunks, int nchunks, double lr, double bias_correction1,
                      double bias_correction2, double beta1, double beta2, double eps, double weight_decay, int amsgrad, frtm_stream_t stream);

/* Batched resize of native-size uint8 training frames / label maps to the training size in one launch each (csrc/frame_resize.hip;
 * replaces the per-frame cv2.resize / F.interpolate of the reference's lib/training_datasets.py:185-195, which run on the CPU).
 * src: DEVICE byte buffer of src_bytes bytes holding n frames one after another at ARBITRARY byte offsets (no alignment is asked of the
 * packer or of src itself).  The table has one row of four 64-bit words per frame and is passed twice: desc_host (HOST memory, checked
 * before the launch: 1 <= h, w <= 16384, the frame inside the buffer, a known mode / an id in 0..255 -- anything else returns
 * FRTM_ERR_ARG without launching) and desc_dev, the same rows in DEVICE memory, which the kernel reads.  1 <= H, W <= 16384.
 *   frtm_resize_frames_u8   rows {offset, h, w, mode}; a frame is `planes` planes of h x w bytes; out (n, planes, H, W) uint8;
 *                           n * planes <= 65535.  FRTM_RESIZE_AREA (cv2.INTER_AREA's role), per axis: src > dst: the mean over the source
 *                           interval [d src/dst, (d + 1) src/dst) with fractional edge coverage; src == dst: the identity (bit-exact);
 *                           src < dst: bilinear, half-pixel centres, replicate border.  FRTM_RESIZE_CUBIC: frtm_bicubic_resize's operator.
 *                           fp32 sums with weights one rounding away from exact, ONE rounding to nearest-even, clamp to 0..255.
 *   frtm_resize_labels_u8   rows {offset, h, w, obj_id}; a frame is one plane; out (n, 1, H, W) uint8 = (src == obj_id) at the source
 *                           index of F.interpolate(mode='nearest'): min(floor(dst * (float(src) / dst_size)), src - 1) in float32. */
#define FRTM_RESIZE_AREA 0
#define FRTM_RESIZE_CUBIC 1
int frtm_resize_frames_u8(const unsigned char* src, size_t src_bytes, const long long* desc_host, const long long* desc_dev, int n, int planes,
                          unsigned char* out, int H, int W, frtm_stream_t stream);
int frtm_resize_labels_u8(const unsigned char* src, size_t src_bytes, const long long* desc_host, const long long* desc_dev, int n,
                          unsigned char* out, int H, int W, frtm_stream_t stream);

/* The way back from a working size (csrc/native_size.hip; Tracker(working_size=...), StreamPool(working_size=...)): native-size label
 * maps and masks from MERGED mask stacks at the working size h x w, for n frames of any native sizes and plane counts in one launch.
 * masks: DEVICE fp32 buffer of mask_elems floats.  The table has one row of seven 64-bit words per frame and is passed twice like the
 * resize tables (table_host is checked and sizes the grid, table_dev is what the kernel reads):
 *   {offset of the frame's first plane in masks (floats), K planes (1 .. 16 = n_obj + 1), native H, native W (1 .. 16384 each),
 *    offset of the frame's H x W label map in labels (bytes), offset of its K x H x W planes in soft (floats) or -1: none,
 *    offset of its K-byte LUT in luts (bytes)}.
 * Per native pixel: m_k = the bilinear sample of plane k (ATen's upsample_bilinear2d, align_corners=False; the plane itself when the sizes
 * agree), arg = the first k with the largest m_k, label = lut[arg] if arg >= 1 and m_arg > 0.5f, else lut[0]; the soft planes are the m_k.
 * On equal sizes the labels are frtm_track_merge's, byte for byte.  K or a native size outside its range returns FRTM_ERR_ARG without
 * launching; a row whose frame does not lie inside the four buffers (mask_elems, label_bytes, soft_elems, lut_bytes) is SKIPPED: nothing
 * of it is read or written.  soft may be NULL when no row asks for planes.  n <= 65535. */
int frtm_masks_to_native(const float* masks, size_t mask_elems, int h, int w, const long long* table_host, const long long* table_dev, int n,
                         unsigned char* labels, size_t label_bytes, float* soft, size_t soft_elems, const unsigned char* luts, size_t lut_bytes,
                         frtm_stream_t stream);

/* frtm_resize_labels_u8 with the id kept: rows {offset, h, w, 0}; out (n, 1, H, W) uint8 = src at the source index of
 * F.interpolate(mode='nearest') (the first-frame label map on its way to the working size). */
int frtm_resize_label_map_u8(const unsigned char* src, size_t src_bytes, const long long* desc_host, const long long* desc_dev, int n,
                             unsigned char* out, int H, int W, frtm_stream_t stream);

/* Decoder frames to planar RGB at one output size, n frames of any sizes, formats and modes in ONE launch (csrc/frame_formats.hip):
 * colour conversion and frtm_resize_frames_u8's operator fused.  src and the two copies of the table as there; a row is eight 64-bit words
 *   {off, h, w, mode, format, pitch, uv_off, 0}.
 * FRTM_FRAME_RGB: three planes of h x w bytes at off (pitch and uv_off ignored): exactly frtm_resize_frames_u8 with planes = 3.
 * FRTM_FRAME_NV12_*: an NV12 surface -- Y plane at off, rows `pitch` bytes apart; interleaved U,V plane at uv_off (uv_off > off + pitch * h
 * expresses a coded height above the picture's), rows `pitch` apart as well, pitch >= 2 * ceil(w / 2).  Source pixel (y, x):
 *   Y = src[off + y * pitch + x], U = src[uv_off + (y >> 1) * pitch + 2 * (x >> 1)], V = the byte after U   (chroma replicated, not interpolated)
 *   yy = Y - y0, u = U - 128, v = V - 128, in int32:
 *   R = clamp(floor((a * yy + rv * v + 32768) / 65536), 0, 255)
 *   G = clamp(floor((a * yy - gu * u - gv * v + 32768) / 65536), 0, 255)
 *   B = clamp(floor((a * yy + bu * u + 32768) / 65536), 0, 255)
 *   format            y0      a      rv     gu     gv      bu      (round(65536 * coefficient) of the standard matrices)
 *   NV12_BT601        16  76309  104597  25675  53279  132201
 *   NV12_BT601_FULL    0  65536   91881  22553  46802  116130
 *   NV12_BT709        16  76309  117489  13975  34925  138438
 *   NV12_BT709_FULL    0  65536  103206  12276  30679  121609
 * out (n, 3, H, W) uint8 = those uint8 planes through frtm_resize_frames_u8's operator, bit for bit (H x W = h x w: the conversion alone).
 * Loads touch [off, off + pitch * h) and [uv_off, uv_off + pitch * ceil(h / 2)) only ([off, off + 3 h w) for FRTM_FRAME_RGB), and of those
 * only picture samples.  Refused with FRTM_ERR_ARG before any launch: a null pointer, n < 1, 3 n > 65535, a size outside 1 .. 16384, an
 * unknown mode or format, pitch < 2 * ceil(w / 2), a range that leaves [0, src_bytes). */
#define FRTM_FRAME_RGB 0
#define FRTM_FRAME_NV12_BT601 1
#define FRTM_FRAME_NV12_BT601_FULL 2
#define FRTM_FRAME_NV12_BT709 3
#define FRTM_FRAME_NV12_BT709_FULL 4
int frtm_frames_to_rgb_u8(const unsigned char* src, size_t src_bytes, const long long* desc_host, const long long* desc_dev, int n,
                          unsigned char* out, int H, int W, frtm_stream_t stream);

/* The way out (csrc/frame_render.hip; ops.render_frames, Tracker.render, StreamPool.render): the tracked objects of n frames of any sizes
 * and formats rendered onto those frames in ONE launch.  The table has one row of FRTM_RENDER_ROW_WORDS 64-bit words per frame and is passed
 * twice like the other frame tables (table_host is checked and sizes the grid, table_dev is what the kernel reads, and every workgroup checks
 * its row again).  Rows carry ADDRESSES: a caller's surfaces are separate allocations.
 *   { format, h, w,  src, src_bytes, src_pitch, src_uv_off,  dst, dst_bytes, dst_pitch, dst_uv_off,
 *     form, answer, answer_bytes, K, lut,  style, soft, edge_alpha, 0 }
 * format FRTM_RENDER_RGB: src / dst are three planes of h x w bytes (pitch and uv_off ignored); FRTM_RENDER_NV12: the Y plane at the address,
 * rows `pitch` bytes apart, interleaved U,V at address + uv_off, rows `pitch` apart as well, pitch >= 2 * ceil(w / 2), uv_off >= pitch * h --
 * frtm_frames_to_rgb_u8's layout, source and destination each with their own pitch and uv_off; a surface spans uv_off + pitch * ceil(h / 2)
 * bytes (3 h w for RGB), which must not exceed its *_bytes.  1 <= h, w <= 16384.  dst is src itself with the same layout (in place) or shares
 * no byte with it, and shares none with the answer.
 * form FRTM_RENDER_LABELS: answer is an h x w uint8 map of object ids (K, lut ignored).  FRTM_RENDER_MASKS: answer is a 4-byte aligned
 * (K, h, w) fp32 MERGED mask stack, 1 <= K <= 16, lut its K bytes plane -> id, decoded by frtm_masks_to_native's rule: arg = the first k
 * with the largest m_k, id = lut[arg] if arg >= 1 and m_arg > 0.5f, else lut[0].  answer_bytes: the bytes available behind answer.
 * style: 256 rows of 4 bytes (c0, c1, c2, a) indexed by object id, in the frame's own channels (R,G,B; or Y,U,V: see below).
 * soft 0 or 1 (FRTM_RENDER_MASKS only); edge_alpha -1 (off) or 0 .. 255 (not with soft).
 *
 * Per pixel, on its three channel bytes s = (s0, s1, s2) -- R,G,B; for NV12 Y and the chroma sample (U, V) of its 2 x 2 block, replicated
 * as by frtm_frames_to_rgb_u8 --, per channel:
 *   mix(s, c, a) = (t + (t >> 8)) >> 8,  t = s * (255 - a) + c * a + 128     ( = round(s + (c - s) * a / 255), half up, for all s, c, a in 0 .. 255 )
 *   hard (soft 0): out = mix(s, c_id, a_id), id the pixel's label, background included.  With edge_alpha on, a pixel whose id is not the
 *     background's (lut[0]; 0 for a label map) uses edge_alpha instead of a_id when at least one of its 4-neighbours INSIDE the picture has
 *     another label (the picture's own border makes no edge).
 *   soft: k* = the first k >= 1 with the largest m_k (a NaN is never the largest), m = fminf(fmaxf(m_k*, 0), 1); no such plane (K = 1,
 *     NaNs only): m = 0.  B = mix(s, c_b, a_b), b = lut[0]; F = mix(s, c_f, a_f), f = lut[k*];
 *     out = (int)rintf(fmaf(m, (float)(F - B), (float)B)): one fused multiply-add, one rounding to nearest even.  m in {0, 1}: the hard rule.
 * NV12 output: Y' is the per-pixel result; chroma sample (j, i) covers the cnt = 1, 2 or 4 picture pixels of rows 2j .. min(2j + 1, h - 1),
 * columns 2i .. min(2i + 1, w - 1): U' = (the sum of their U results + cnt / 2) / cnt, V' likewise.  A block in which nothing changes keeps
 * its bytes; a style whose every a is 0 is the identity.  Loads and stores touch picture samples only, in src and in dst: never a byte of the
 * row padding or of the rows between the picture and the coded height.
 *
 * The kernel knows no colour matrix: for an NV12 frame the caller converts its RGB palette once, by the forward formula that belongs to the
 * inverse one of frtm_frames_to_rgb_u8 (coefficients round(65536 * the standard forward coefficient), >> the arithmetic shift):
 *   Y = clamp(y0 + ((yr R + yg G + yb B + 32768) >> 16)),  U = clamp(128 + ((ur R + ug G + ub B + 32768) >> 16)),
 *   V = clamp(128 + ((vr R + vg G + vb B + 32768) >> 16)),  clamp to 0 .. 255
 *   matrix and range    y0     yr     yg    yb      ur      ug     ub     vr      vg     vb
 *   BT601               16  16829  33039  6416   -9714  -19071  28784  28784  -24103  -4681
 *   BT601_FULL           0  19595  38470  7471  -11058  -21710  32768  32768  -27439  -5329
 *   BT709               16  11966  40254  4064   -6596  -22189  28784  28784  -26145  -2639
 *   BT709_FULL           0  13933  46871  4732   -7509  -25259  32768  32768  -29763  -3005
 * Refused with FRTM_ERR_ARG and a message before any launch: a null table or address, n outside 1 .. 65535, an unknown format or form, a
 * size outside 1 .. 16384, K outside 1 .. 16, a pitch below a chroma row, a surface or an answer that leaves its buffer, a misaligned mask
 * stack, a partial overlap, soft with a label map or with edge_alpha. */
#define FRTM_RENDER_RGB 0
#define FRTM_RENDER_NV12 1
#define FRTM_RENDER_LABELS 0
#define FRTM_RENDER_MASKS 1
#define FRTM_RENDER_ROW_WORDS 20
int frtm_render_frames_u8(const long long* table_host, const long long* table_dev, int n, frtm_stream_t stream);

/* The numbers a program needs to ACT on the answer (csrc/object_report.hip; ops.describe_frames, Tracker.describe, StreamPool.describe): the
 * tracked objects of n frames of any sizes measured in ONE launch, label maps and mask stacks mixed.  The conventions are
 * frtm_render_frames_u8's: the table is passed twice (table_host is checked and sizes the grid, table_dev is what the kernels read, and every
 * workgroup checks its row again), rows carry ADDRESSES, everything is enqueued on `stream` and nothing synchronises.  A row is
 * FRTM_OBJECT_ROW_WORDS 64-bit words:
 *   { form, h, w, answer, answer_bytes, K, ids, 0 }
 * form FRTM_OBJECT_LABELS: answer is an h x w uint8 map of object ids; ids: the address of the K DISTINCT ids to measure (a precondition: the
 * host cannot read device bytes; if an id is listed twice the first slot that lists it takes the pixel).  FRTM_OBJECT_MASKS: answer is a 4-byte
 * aligned (K, h, w) fp32 MERGED mask stack, ids its K bytes plane -> id.  1 <= K <= 16, 1 <= h, w <= 16384; answer_bytes: the bytes available
 * behind answer.
 * The slot of a pixel.  Stack: the decoded plane of frtm_masks_to_native's rule: arg = the first k with the largest m_k (a NaN never wins), slot
 * = arg if arg >= 1 and m_arg > 0.5f, else 0.  Label map: the index of the pixel's id in ids; a pixel whose id is not listed has no slot.
 * The label of a pixel (for edges): the decoded plane, or the id of a label map -- an unlisted id is still another label.
 * out: n x 16 x FRTM_OBJECT_WORDS 64-bit words, frame-major then slot; out_words (the words available behind out) must be at least that many.
 * The words of slot s < K of a frame (slots s >= K: twelve zeros):
 *   0      area     pixels of the slot
 *   1 .. 4 x_min, y_min, x_max, y_max   the inclusive box; of an empty slot w, h, -1, -1
 *   5, 6   sum_x, sum_y   sums of the coordinates of the slot's pixels (centroid = sum / area)
 *   7      edge     pixels of the slot with at least one 4-neighbour INSIDE the picture that has another label (the renderer's edge rule, for
 *                   every slot, slot 0 included; the picture's own border makes no edge)
 *   8      border   pixels of the slot on row 0, row h - 1, column 0 or column w - 1 (a corner counts once)
 *   9      conf     stacks: the sum over the slot's pixels of q(m_slot), q(m) = (long long)rintf(255.0f * fminf(fmaxf(m, 0.0f), 1.0f)), a NaN
 *                   gives 0; label maps: 0
 *   10     mass     stacks: the sum over ALL pixels of q(m_s) of plane s (255 x the soft area: above zero while a fading object's area is 0
 *                   already); label maps: 0
 *   11     id       ids[s]
 * All accumulation is in integers (64-bit in memory: sum_x reaches 2^42, conf 2^36), hence independent of order and deterministic; no float
 * atomics.  A call enqueues exactly TWO operations on `stream`: the kernel that writes the start of every word (zeros, the empty box, the ids)
 * and the kernel that measures, with one integer atomic per workgroup and word.  Loads touch picture samples and the K id bytes only; stores
 * touch the n x 16 x 12 words only.
 * Refused with FRTM_ERR_ARG and a message before anything is enqueued, out untouched: a null table, address or out, n outside 1 .. 65535, an
 * unknown form, a size outside 1 .. 16384, K outside 1 .. 16, an answer that leaves answer_bytes, a misaligned stack, out_words too small, a
 * non-zero last word. */
#define FRTM_OBJECT_LABELS 0
#define FRTM_OBJECT_MASKS 1
#define FRTM_OBJECT_ROW_WORDS 8
#define FRTM_OBJECT_SLOTS 16
#define FRTM_OBJECT_WORDS 12
int frtm_describe_frames(const long long* table_host, const long long* table_dev, int n, long long* out, size_t out_words,
                         frtm_stream_t stream);

/* The tracked masks in the form consumers of segmentation read -- COCO run lengths, one list per object -- coded on the device
 * (csrc/mask_runs.hip; ops.encode_frames, Tracker.encode, StreamPool.encode).  The conventions are frtm_describe_frames's: the table is passed
 * twice (table_host is checked and sizes the grid and the workspace, table_dev is what the kernels read, and every workgroup checks its row
 * again), rows carry ADDRESSES, everything is enqueued on `stream`, nothing synchronises and nothing is allocated.  The row is
 * frtm_describe_frames's row word for word -- { form, h, w, answer, answer_bytes, K, ids, 0 }, the same forms and limits -- so a table built
 * for one call serves the other, and the slot of a pixel is that call's slot (stack: the decoded plane; label map: the index of its id in ids,
 * none when not listed).  Slot s of a frame is the binary mask b_s(y, x) = [slot(y, x) == s].
 * The code of a slot.  With N = h w and p = x h + y (column-major, as COCO scans): the lengths of the maximal runs of equal bits of b_s(p),
 * p = 0 .. N - 1, in order, STARTING WITH A RUN OF ZEROS: the first count is 0 when b_s(0) = 1.  With B the number of p in 1 .. N - 1 where
 * b_s(p) != b_s(p - 1) the list has B + 1 + b_s(0) entries and they sum to N.  p - 1 of a pixel in row 0 is the last row of the previous
 * column: a run continues from the bottom of a column into the top of the next.  All zeros: [N]; all ones: [0, N];
 * h = 3, w = 4, rows 0110 / 0100 / 1101: [2, 5, 4, 1].
 * heads: n x 16 x FRTM_RUNS_HEAD_WORDS 64-bit words, frame-major then slot (head_words, the words available, at least that many):
 *   { count, offset, area, id }   count: the length of the slot's list; offset: where it starts in runs; area: the sum of its odd-indexed
 *                                 counts (= word 0 of frtm_describe_frames); id: ids[s].  Slots s >= K: four zeros.
 * The layout is fixed: offset(frame 0, slot 0) = 0 and every following (frame, slot) in use starts where the one before it ends; `needed` is
 * offset + count of the last slot in use.  Element j of that concatenation is stored in runs[j] iff j < run_capacity: heads always holds the
 * TRUE counts and offsets, a slot is complete iff offset + count <= run_capacity, and runs at or beyond min(needed, run_capacity) is not
 * touched.  Every word of heads and every stored element is an exact function of the inputs: no atomics, no float arithmetic after the decode,
 * no position that depends on an order of arrival; two calls give the same bytes.
 * work: frtm_encode_work_bytes(table_host, n, run_capacity) bytes, 8-byte aligned; its content is this call's alone.  (That function runs on
 * the host without a device; 0 and a message for a table, an n or a run_capacity that frtm_encode_frames would refuse.  The size is
 * 4 (16 n + 2 n C) with C = max over the frames of K w ceil(h / 64): two words per (slot, column, 64-row segment).  run_capacity is checked but
 * does not enter: the positions of the boundaries are never stored.)
 * A call enqueues exactly FOUR operations on `stream`, whatever n, the sizes and the content: the kernel that counts every cell's boundaries,
 * the scan of every slot's cells (which writes count, area and id), the scan of the slots (offsets and every list's last element), and the
 * kernel that walks the pixels again and stores the run lengths.  Loads touch picture samples and the K id bytes only; stores touch heads,
 * runs[0 .. min(needed, run_capacity)) and work only.
 * Refused with FRTM_ERR_ARG and a message before anything is enqueued, outputs untouched: everything frtm_describe_frames refuses for its
 * table, a null or misaligned heads / runs / work, head_words < n x 16 x 4, work_bytes below frtm_encode_work_bytes, run_capacity < 1 or
 * > 2^40. */
#define FRTM_RUNS_HEAD_WORDS 4
size_t frtm_encode_work_bytes(const long long* table_host, int n, size_t run_capacity);
int frtm_encode_frames(const long long* table_host, const long long* table_dev, int n, long long* heads, size_t head_words,
                       unsigned int* runs, size_t run_capacity, void* work, size_t work_bytes, frtm_stream_t stream);

/* The answer cleaned on the device (csrc/object_parts.hip; ops.clean_frames, Tracker.clean, StreamPool.clean): every object of n frames of any
 * sizes, label maps and mask stacks mixed, split into its connected parts, the parts measured, a keep rule applied and a cleaned uint8 label
 * map written per frame -- an answer frtm_render_frames_u8, frtm_describe_frames and frtm_encode_frames accept as it is.  The conventions are
 * frtm_describe_frames's: the table is passed twice (table_host is checked and sizes the grid, table_dev is what the kernels read, and every
 * workgroup checks its row again), rows carry ADDRESSES, everything is enqueued on `stream`, nothing synchronises and nothing is allocated.
 * A row is FRTM_PARTS_ROW_WORDS 64-bit words:
 *   { form, h, w, answer, answer_bytes, K, ids, 0,   labels, labels_bytes, components, components_bytes, work, work_bytes, 0, 0 }
 * The first 8 words are frtm_describe_frames's row word for word, with its forms, limits and check.  labels: the h x w uint8 cleaned map
 * (labels_bytes >= h w available; it may not overlap the answer); components: 0 for none, or a 4-byte aligned h x w int32 map
 * (components_bytes >= 4 h w); work: this frame's part of the work buffer, 16-byte aligned, work_bytes >= 16 ceil((128 + 8 h w) / 16): 16 packed
 * 64-bit words (a slot's largest part), then two int32 per pixel -- the parent (finally: the name) and the area at the root.
 * frtm_clean_work_bytes(table_host, n) is the sum of that over the frames, so the parts laid out one behind the other fit; it reads the first
 * 8 words of every row only, runs on the host without a device, and returns 0 and a message for a table or an n frtm_clean_frames would refuse.
 * The slot of a pixel is frtm_describe_frames's slot (stack: the decoded plane, a NaN never wins, threshold 0.5; label map: the index of its
 * id in ids, none when not listed).  The rule, per call: connectivity 4 or 8; min_area 1 .. 2^28; largest_only 0 or 1; fill 0 .. 255.
 * Parts.  A part is a maximal set of pixels of one slot joined by 4- (or 8-) neighbour steps inside the picture; its NAME is the smallest
 * y w + x among its pixels; pixels without a slot belong to no part.  Slot s is RULED when ids[s] != fill.  A part of a ruled slot is kept iff
 * its area >= min_area and (largest_only is 0 or it is its slot's largest part, ties to the smaller name); the parts of an unruled slot (the
 * background) are all kept, and counted all the same.
 * Outputs.  labels: ids[slot] where the pixel's part is kept, else fill; a label-map pixel without a slot keeps its input byte.  components:
 * the name of the pixel's part, -1 without a slot.  words: n x 16 x FRTM_PARTS_WORDS 64-bit words, frame-major then slot (word_count, the
 * words available, at least that many); slot s < K (slots s >= K: twelve zeros):
 *   0  parts         parts of the slot                  1  kept       parts kept
 *   2  area          pixels of the slot (= word 0 of frtm_describe_frames)      3  kept_area  pixels kept
 *   4  largest_area  area of the largest part           5  largest_name   its name; -1 for an empty slot
 *   6 .. 9  x_min, y_min, x_max, y_max of the largest part, inclusive; of an empty slot w, h, -1, -1
 *   10 ruled  0 or 1                                    11 id         ids[s]
 * status: n 64-bit words (status_count at least n): 0, or the bits of the phases in which a bounded loop reached its cap (1 local, 2 seam,
 * 4 flatten) -- by the bounds in object_parts.hip that cannot happen; a frame with a non-zero status has unspecified outputs.
 * All accumulation is in integers and no output depends on an order of arrival: the root of a part is its smallest pixel whatever the order
 * of the unions, areas are integer sums, and the largest part is ONE 64-bit unsigned maximum over area << 32 | (2^31 - 1 - name).  Two calls
 * give the same bytes.  A call enqueues exactly SIX operations on `stream`, whatever n, the sizes and the content:
 *   begin    the start of every word (zeros, the empty box, ruled, id), status and the packed words
 *   local    per FRTM_PARTS_TILE_H x FRTM_PARTS_TILE_W tile: the slots decoded (kept in labels for the later passes), row runs from ballots,
 *            union-find in LDS; parent[p] = the tile's smallest pixel of p's part, area = the part's pixels in the tile (at that pixel)
 *   seam     every pixel on a tile seam joined with its neighbours across the seam: lock-free unions, agent-scope atomics only
 *   flatten  parent[p] = the root; the tile-local areas added to the root's
 *   slots    parts, area and the packed maximum per slot, reduced per workgroup, one integer atomic per workgroup and word
 *   write    labels, components, kept, kept_area and the largest part's box, reduced per workgroup likewise
 * No grid barrier, no flag a workgroup waits on, no loop that runs until convergence.  Loads touch picture samples, the K id bytes, labels
 * and work; stores touch labels, components (when given), work, words and status only.
 * Refused with FRTM_ERR_ARG and a message before anything is enqueued, outputs untouched: everything frtm_describe_frames refuses for the
 * first 8 words, a null, misaligned or too small labels / components / work / words / status, labels overlapping the answer, non-zero last
 * words, n outside 1 .. 65535, connectivity other than 4 or 8, min_area outside 1 .. 2^28, largest_only other than 0 or 1, fill outside
 * 0 .. 255. */
#define FRTM_PARTS_ROW_WORDS 16
#define FRTM_PARTS_WORDS 12
#define FRTM_PARTS_TILE_H 32
#define FRTM_PARTS_TILE_W 64
size_t frtm_clean_work_bytes(const long long* table_host, int n);
int frtm_clean_frames(const long long* table_host, const long long* table_dev, int n, int connectivity, long long min_area, int largest_only,
                      int fill, long long* words, size_t word_count, long long* status, size_t status_count, frtm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FRTM_HIP_H */
