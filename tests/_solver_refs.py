"""Plain torch definitions of the chain-form solver kernels (csrc/joint_fit.hip, the CG and stencil part of csrc/target_model.hip), one per
C entry point, written from the contracts of include/frtm_hip.h with no project code: F.conv2d, F.conv_transpose2d, einsum and an explicit
padded-shift stencil.  Every function works in the dtype and on the device of its arguments, so the same text serves as the float64
reference on the CPU and as the fp32 yardstick of the gate on the GPU.  tests/test_solver_refs.py pins them to oracle/cpu_ref.py.

Layouts are those of the C side: the projection stored transposed, (Cin, c); filters as (C, 9); maps as (N, h, w); D pixel-major (N, h*w, C);
weight-gradient slabs (N*parts, C*9); partial score maps (splits+1, N, h*w); banks of dot-product partials (FRTM_CG_BLOCKS, 2).

The five CG kernels are written as literal one-launch state transitions: (x, r, r_prev, p, q, state[8], the bank read) -> everything the launch
writes.  A transition returns new tensors and leaves its arguments alone.
"""
import torch
import torch.nn.functional as F

CG_BLOCKS = 64          # FRTM_CG_BLOCKS


# ---------------------------------------------------------------------------------------------------------------------------------
# operator pieces
# ---------------------------------------------------------------------------------------------------------------------------------
def conv3x3(X, f):
    """frtm_filter_scores.  X (N,C,h,w), f (C,9) -> (N,h,w): out[n,y,x] = sum_c sum_{dy,dx} X[n,c,y+dy-1,x+dx-1] f[c,dy,dx]."""
    return F.conv2d(X, f.reshape(1, -1, 3, 3), padding=1)[:, 0]


def conv1x1(X, pT):
    """X (N,Cin,h,w), pT (Cin,c) (the projection as stored: transposed) -> (N,c,h,w)."""
    return torch.einsum('nihw,ic->nchw', X, pT)


def filter_scores2(X1, f1, X2, f2):
    """frtm_filter_scores2."""
    return conv3x3(X1, f1) + conv3x3(X2, f2)


def channel_groups(C, splits):
    """The channel groups of the split score passes: `splits` contiguous groups of ceil(C / splits) channels, the last ones short or empty."""
    per = -(-C // splits)
    return [(min(C, k * per), min(C, (k + 1) * per)) for k in range(splits)]


def filter_scores_split(X, f, splits):
    """frtm_filter_scores_split.  -> (splits, N, h*w); an empty group gives a zero map."""
    N, C, h, w = X.shape
    out = X.new_zeros(splits, N, h * w)
    for k, (lo, hi) in enumerate(channel_groups(C, splits)):
        if hi > lo:
            out[k] = conv3x3(X[:, lo:hi], f[lo:hi]).reshape(N, h * w)
    return out


def joint_scores_composed(X, K, Z, p2, splits):
    """frtm_joint_scores_composed.  Maps 0..splits-1: channel groups of X under K (Cx,9); map `splits`: Z under p2 (Cz,9)."""
    N, _, h, w = X.shape
    return torch.cat([filter_scores_split(X, K, splits), conv3x3(Z, p2).reshape(1, N, h * w)])


def stencil(B, c, sw, s):
    """frtm_stencil.  B (N,9,h,w), c (N,h,w) or None, sw (N), s (N,h,w):
    t[n,i,j] = sw[n] (sum_{di,dj} B[n,(di,dj),i,j] s[n,i+di,j+dj] - c[n,i,j]), s zero outside the map."""
    N, h, w = s.shape
    sp = F.pad(s, (1, 1, 1, 1))
    acc = torch.zeros_like(s)
    for a in range(3):
        for b in range(3):
            acc = acc + B[:, a * 3 + b] * sp[:, a:a + h, b:b + w]
    if c is not None:
        acc = acc - c
    return sw.view(N, 1, 1) * acc


def stencil_sum(B, c, sw, partials, h, w):
    """frtm_stencil_sum.  partials (nsum, N, h*w), added in the order 0, 1, ..."""
    s = partials[0]
    for k in range(1, partials.shape[0]):
        s = s + partials[k]
    return stencil(B, c, sw, s.reshape(-1, h, w))


def filter_wgrad(X, t):
    """frtm_filter_wgrad summed over the parts of a sample.  X (N,C,h,w), t (N,h,w) -> (N, C*9):
    g[n, c*9+dy*3+dx] = sum_{y,x} X[n,c,y+dy-1,x+dx-1] t[n,y,x]."""
    N, C, h, w = X.shape
    Xp = F.pad(X, (1, 1, 1, 1))
    g = X.new_zeros(N, C, 9)
    for dy in range(3):
        for dx in range(3):
            g[:, :, dy * 3 + dx] = torch.einsum('nchw,nhw->nc', Xp[:, :, dy:dy + h, dx:dx + w], t)
    return g.reshape(N, C * 9)


def filter_igrad(t, f):
    """frtm_filter_igrad, pix_major.  t (N,h,w), f (C,9) -> D (N, h*w, C): D[n,(y,x),c] = sum_{dy,dx} f[c,dy,dx] t[n,y-dy+1,x-dx+1]."""
    N, h, w = t.shape
    D = F.conv_transpose2d(t[:, None], f.reshape(1, -1, 3, 3), padding=1)
    return D.reshape(N, -1, h * w).transpose(1, 2).contiguous()


def joint_mid(s, B, cm, sw, Z, w2):
    """frtm_joint_mid.  -> (slabs summed over the parts of a sample (N, C*9), D (N, h*w, C))."""
    t = stencil(B, cm, sw, s)
    return filter_wgrad(Z, t), filter_igrad(t, w2)


def reduce_slabs(slabs, nslab, stride, n):
    """sum_k slabs[k*stride + i], i < n, over a flat buffer, in the order k = 0, 1, ..."""
    flat = slabs.reshape(-1)
    acc = flat[:n].clone()
    for k in range(1, nslab):
        acc = acc + flat[k * stride:k * stride + n]
    return acc


def vec_reduce_slabs(slabs, nslab, stride, n, lam2, p, sign):
    """frtm_vec_reduce_slabs.  q = sign (sum_k slabs[k*stride + i] + lam2 p[i]); p may be None."""
    acc = reduce_slabs(slabs, nslab, stride, n)
    if p is not None:
        acc = acc + lam2 * p
    return sign * acc


def vec_axpy(y, a, x):
    """frtm_vec_axpy."""
    return y + a * x


def joint_q_pq(g1, lam1, slabs, nslab, stride, n2, lam2, p1, p2, sign):
    """frtm_joint_q_pq.  q = sign [g1 + lam1 p1 | sum of the slabs + lam2 p2]."""
    return torch.cat([sign * (g1 + lam1 * p1), sign * (reduce_slabs(slabs, nslab, stride, n2) + lam2 * p2)])


def joint_compose(p1, w2):
    """frtm_joint_compose.  p1 (Cin,c), w2 (c,9) -> K (Cin,9)."""
    return p1 @ w2


def joint_expand(G, w2, lam, p1, sign):
    """frtm_joint_expand.  G (nslab,Cin,9) -> q1 (Cin,c) = sign ((sum of the slabs) w2^T + lam p1)."""
    acc = G[0]
    for k in range(1, G.shape[0]):
        acc = acc + G[k]
    return sign * (acc @ w2.t() + lam * p1)


def joint_q_pq_composed(GX, w2, lam1, slabs, nslab, stride, n2, lam2, p1, p2, sign):
    """frtm_joint_q_pq_composed.  GX (nslabX,Cin,9), p1 (Cin,c) -> q = [q1 as joint_expand, flat | sign (sum of the slabs + lam2 p2)]."""
    return torch.cat([joint_expand(GX, w2, lam1, p1, sign).reshape(-1), sign * (reduce_slabs(slabs, nslab, stride, n2) + lam2 * p2)])


def dot_terms(p, q):
    """The terms of <p,q>; their sum is what a bank of partials adds up to, the sum of their magnitudes what its rounding scales with."""
    return p * q


# ---------------------------------------------------------------------------------------------------------------------------------
# whole operators in low-resolution form (B = U^T W^2 U, c = U^T W^2 y, sw the sample weights)
# ---------------------------------------------------------------------------------------------------------------------------------
def _joint_grad(X, Z, w2, sw_t):
    """[g1 (Cin,c) flat | g2 (c*9)] of the one-channel map t: g2 = wgrad(Z,t) over all samples, g1 = X^T igrad(t,w2)."""
    N, Cin, h, w = X.shape
    g2 = filter_wgrad(Z, sw_t).sum(0)
    D = filter_igrad(sw_t, w2)                                    # (N, hw, c)
    g1 = torch.einsum('nip,npc->ic', X.reshape(N, Cin, h * w), D)
    return g1.reshape(-1), g2


def joint_rhs(X, w1T, w2, B, c, sw, lam1, lam2):
    """b = -(J^T f(x) + lam x) of the joint problem at (w1T (Cin,c), w2 (c,9)), flat [Cin*c | c*9]."""
    Z = conv1x1(X, w1T)
    g1, g2 = _joint_grad(X, Z, w2, stencil(B, c, sw, conv3x3(Z, w2)))
    return torch.cat([-(g1 + lam1 * w1T.reshape(-1)), -(g2 + lam2 * w2.reshape(-1))])


def joint_A(X, w1T, w2, B, sw, lam1, lam2, p1, p2):
    """q = J^T J p + lam p of the joint problem linearised at (w1T, w2); p1 (Cin,c), p2 (c,9)."""
    Z = conv1x1(X, w1T)
    s = conv3x3(conv1x1(X, p1), w2) + conv3x3(Z, p2)
    g1, g2 = _joint_grad(X, Z, w2, stencil(B, None, sw, s))
    return torch.cat([g1 + lam1 * p1.reshape(-1), g2 + lam2 * p2.reshape(-1)])


def filter_rhs(X, w2, B, c, sw, lam):
    """b of the filter-only problem: -(wgrad(X, sw (B (X * w2) - c)) + lam w2)."""
    return -(filter_wgrad(X, stencil(B, c, sw, conv3x3(X, w2))).sum(0) + lam * w2.reshape(-1))


def filter_A(X, p, B, sw, lam):
    """q of the filter-only problem: wgrad(X, sw B (X * p)) + lam p."""
    return filter_wgrad(X, stencil(B, None, sw, conv3x3(X, p))).sum(0) + lam * p.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# CG kernels: one launch each.  state = [rho, alpha, beta, pq, rho_new, rho2, -, -]; a bank is (CG_BLOCKS, 2): word 0 and word 1 of each
# block's partial sums; a launch that reads a bank reads the two column sums.
# ---------------------------------------------------------------------------------------------------------------------------------
def bank(t0, t1=None):
    """(CG_BLOCKS, 2) partials of the term vectors t0 / t1 (None: zeros) over contiguous slices of ceil(n / CG_BLOCKS) elements."""
    n = t0.numel()
    per = -(-n // CG_BLOCKS)
    out = t0.new_zeros(CG_BLOCKS, 2)
    for k, t in enumerate((t0, t1)):
        if t is not None:
            out[:, k] = F.pad(t, (0, CG_BLOCKS * per - n)).reshape(CG_BLOCKS, per).sum(1)
    return out


def _inv_m(v, n1, invM1, invM2):
    m = torch.full_like(v, invM2)
    m[:n1] = invM1
    return m


def cg_begin(b, r_prev, n1, invM1, invM2, has_p):
    """frtm_cg_begin -> (r, bank 1): r = b; partials of <r, M^-1 r> and (has_p) <r_prev, M^-1 r>, else zeros."""
    z = b * _inv_m(b, n1, invM1, invM2)
    return b.clone(), bank(b * z, r_prev * z if has_p else None)


def cg_direction(r, p, n1, invM1, invM2, has_p, apply_dff, fletcher_reeves, dff, state, bank1):
    """frtm_cg_direction -> (p, state): rho_new and rho2 from bank 1, rho1 = state[0] (/ dff if apply_dff);
    beta = clamp(fletcher_reeves ? rho_new / rho1 : (rho_new - rho2) / rho1, 0); p = z + beta p (z when not has_p; beta = 0 then);
    state[4] = rho_new, state[2] = beta."""
    rho_new, rho2 = bank1[:, 0].sum(), bank1[:, 1].sum()
    beta = torch.zeros_like(rho_new)
    if has_p:
        rho1 = state[0] / dff if apply_dff else state[0]
        v = rho_new / rho1 if fletcher_reeves else (rho_new - rho2) / rho1
        beta = torch.where(v < 0, torch.zeros_like(v), v)
    z = r * _inv_m(r, n1, invM1, invM2)
    st = state.clone()
    st[4], st[2] = rho_new, beta
    return (z + p * beta if has_p else z), st


def cg_pq(p, q, r):
    """frtm_cg_pq -> bank 0: partials of <p,q> and, with r, of <p,r>."""
    return bank(p * q, None if r is None else p * r)


def cg_update(x, r, r_prev, p, q, n1, invM1, invM2, first, last, standard_alpha, state, bank0):
    """frtm_cg_update -> (x, r, r_prev, state, bank 1): alpha = (standard_alpha ? state[4] : <p,r>) / <p,q> from bank 0; r_prev = r;
    x = first ? alpha p : x + alpha p; r -= alpha q unless last; bank 1 = partials of <r, M^-1 r> and <r_prev, M^-1 r> with the new r;
    state[0] = state[4], state[1] = alpha."""
    pq = bank0[:, 0].sum()
    alpha = (state[4] if standard_alpha else bank0[:, 1].sum()) / pq
    xn = p * alpha if first else x + p * alpha
    rn = r if last else r - q * alpha
    z = rn * _inv_m(rn, n1, invM1, invM2)
    st = state.clone()
    st[0], st[1] = state[4], alpha
    return xn, rn.clone(), r.clone(), st, bank(rn * z, r * z)


def cg_step_small(slabs, nslab, stride, lam2, x, r, r_prev, p, n, invM, first, last, standard_alpha, fletcher_reeves, state):
    """frtm_cg_step_small -> (x, r, r_prev, p, q, state), one CG iteration of an n <= 1024 problem whose direction p and rho (state[4])
    a frtm_cg_direction launch or the previous step left:
    q = sum of the slabs + lam2 p; alpha = (standard_alpha ? state[4] : <p,r>) / <p,q>; r_prev = r; x = first ? alpha p : x + alpha p.
    Not last: r -= alpha q, then the next direction: beta = clamp((rho' [- <r_prev,z>]) / rho, 0) with z = M^-1 r, rho' = <r,z>, rho = state[4];
    p = z + beta p; state[0] = rho, state[4] = rho', state[1] = alpha, state[2] = beta.
    Last: r and p stay, state[0] = rho (the run's last rho, where the next run's frtm_cg_direction looks for it), state[1] = alpha; state[4]
    and state[2] stay."""
    q = reduce_slabs(slabs, nslab, stride, n) + lam2 * p
    rho = state[4]
    alpha = (rho if standard_alpha else (p * r).sum()) / (p * q).sum()
    xn = p * alpha if first else x + p * alpha
    st = state.clone()
    st[0], st[1] = rho, alpha
    if last:
        return xn, r.clone(), r.clone(), p.clone(), q, st
    rn = r - q * alpha
    z = rn * invM
    rho_new, rho2 = (rn * z).sum(), (r * z).sum()
    v = rho_new / rho if fletcher_reeves else (rho_new - rho2) / rho
    beta = torch.where(v < 0, torch.zeros_like(v), v)
    st[4], st[2] = rho_new, beta
    return xn, rn, r.clone(), z + p * beta, q, st


# ---------------------------------------------------------------------------------------------------------------------------------
# the launches of one run_CG call composed (model/optimizer.py: run_CG), for tests/test_solver_refs.py
# ---------------------------------------------------------------------------------------------------------------------------------
class CGChain:
    """Solver state (r_prev, p, state[8], has_p) carried over Gauss-Newton iterations, advanced by the transition functions alone.
    apply_A(p) -> q for the multi-kernel sequence; slabs_of(p) -> (slabs, nslab, stride, lam2) for the step-small sequence."""

    def __init__(self, n1, n2, m1, m2, fletcher_reeves, standard_alpha, dff, dtype=torch.float64):
        self.n1, self.n2, self.im1, self.im2 = n1, n2, 1.0 / m1, (1.0 / m2 if n2 else 1.0)
        self.fr, self.std, self.dff = int(fletcher_reeves), int(standard_alpha), float(dff)
        n = n1 + n2
        self.r_prev, self.p = torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
        self.state = torch.zeros(8, dtype=dtype)
        self.state[0] = 1.0
        self.has_p = False

    def _start(self, b):
        if self.dff == 0:
            self.state[0] = 1.0
            self.has_p = False
        apply_dff = int(self.has_p and self.dff != 0)
        r, bank1 = cg_begin(b, self.r_prev, self.n1, self.im1, self.im2, int(self.has_p and not self.fr))
        return r, bank1, apply_dff, (self.dff if self.dff != 0 else 1.0)

    def run_multi(self, b, apply_A, num_iter):
        r, bank1, apply_dff, dff = self._start(b)
        x = torch.zeros_like(b)
        for ii in range(num_iter):
            self.p, self.state = cg_direction(r, self.p, self.n1, self.im1, self.im2, int(self.has_p), apply_dff if ii == 0 else 0, self.fr, dff,
                                              self.state, bank1)
            self.has_p = True
            q = apply_A(self.p)
            bank0 = cg_pq(self.p, q, None if self.std else r)
            x, r, self.r_prev, self.state, bank1 = cg_update(x, r, self.r_prev, self.p, q, self.n1, self.im1, self.im2, int(ii == 0),
                                                             int(ii == num_iter - 1), self.std, self.state, bank0)
        return x

    def run_small(self, b, slabs_of, num_iter):
        assert self.n2 == 0
        r, bank1, apply_dff, dff = self._start(b)
        x = torch.zeros_like(b)
        self.p, self.state = cg_direction(r, self.p, self.n1, self.im1, self.im2, int(self.has_p), apply_dff, self.fr, dff, self.state, bank1)
        self.has_p = True
        for ii in range(num_iter):
            slabs, nslab, stride, lam2 = slabs_of(self.p)
            x, r, self.r_prev, self.p, _, self.state = cg_step_small(slabs, nslab, stride, lam2, x, r, self.r_prev, self.p, self.n1, self.im1,
                                                                      int(ii == 0), int(ii == num_iter - 1), self.std, self.fr, self.state)
        return x


# ---------------------------------------------------------------------------------------------------------------------------------
# the dense problem of the short solves (tests/test_solver_refs.py asserts that it tells the CG flags apart;
# tests/test_solver_kernels_gpu.py runs GaussNewtonCG.run on it)
# ---------------------------------------------------------------------------------------------------------------------------------
SOLVE_SCHEDULE = (3, 4, 2)
SOLVE_LAYOUTS = {'small': (864, 0, 0.25, 1.0), 'multi': (1000, 37, 0.25, 4.0)}          # n1, n2, diag M1, diag M2
SOLVE_LAM = 0.75


def spd_problem(n, seed):
    """fp32 values: A0 (n,n) symmetric with eigenvalues 1 - lam .. 10 - lam (so that A = A0 + lam I has 1 .. 10) and one independent
    right-hand side per Gauss-Newton iteration of SOLVE_SCHEDULE."""
    g = torch.Generator().manual_seed(seed)
    Q, _ = torch.linalg.qr(torch.randn(n, n, generator=g, dtype=torch.float64))
    A0 = (Q * (torch.linspace(1.0, 10.0, n, dtype=torch.float64) - SOLVE_LAM)) @ Q.t()
    A0 = A0.float()
    A0 = ((A0 + A0.t()) * 0.5).contiguous()
    return A0, [torch.randn(n, generator=g) for _ in SOLVE_SCHEDULE]


class DenseProblemRef:
    """The dense problem for oracle.cpu_ref.GaussNewtonCGRef: linearize returns the k-th right-hand side, whatever x is."""

    def __init__(self, A0, rhs, n1, m1, m2):
        self.A0, self.rhs, self.n1, self.diag_M, self.k = A0, rhs, n1, [m1, m2], 0

    def initialize(self):
        pass

    def _split(self, v):
        return [v[:self.n1].clone(), v[self.n1:].clone()]

    def linearize(self, x):
        self.k += 1
        return self._split(self.rhs[self.k - 1])

    def A(self, p):
        v = torch.cat(p)
        return self._split(self.A0 @ v + SOLVE_LAM * v)

    def ip(self, a, b):
        return torch.cat(a) @ torch.cat(b)

    def M1(self, x):
        return [t / m for t, m in zip(x, self.diag_M)]


def dense_reference(cpu_ref, A0, rhs, layout, fletcher_reeves, standard_alpha, dff, dtype):
    """GaussNewtonCGRef over SOLVE_SCHEDULE in `dtype` -> the accumulated variable after each Gauss-Newton iteration."""
    n1, n2, m1, m2 = layout
    pr = DenseProblemRef(A0.to(dtype), [b.to(dtype) for b in rhs], n1, m1, m2)
    x = [torch.zeros(n1, dtype=dtype), torch.zeros(n2, dtype=dtype)]
    opt = cpu_ref.GaussNewtonCGRef(pr, x, fletcher_reeves=fletcher_reeves, standard_alpha=standard_alpha, direction_forget_factor=dff)
    out = []
    for it in SOLVE_SCHEDULE:
        opt.run((it,))
        out.append(torch.cat(x).clone())
    return out
