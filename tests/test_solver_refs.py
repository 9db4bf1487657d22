"""CPU side of the per-kernel checks of the chain-form solver (csrc/joint_fit.hip, the CG and stencil part of csrc/target_model.hip): the
references of tests/_solver_refs.py are pinned here, so that a wrong reference cannot pass as a right kernel.

(a) The low-resolution joint operator and the filter operator (b and A p) equal oracle.cpu_ref.InitProblemRef / UpdateProblemRef -- the
    reference's hi-res form -- on one small problem with real hinge pixel weights, B and c from oracle.cpu_ref.lowres_normal: rel-to-max
    below 1e-5 in fp32.  This catches tap orientation, sign and transposition errors; it is not a precision test.
(b) The igrad / conv and wgrad / conv pairs are adjoint in float64 to 1e-12.
(c) The CG transition functions, composed as model/optimizer.py composes the launches -- once as the multi-kernel sequence, once as the
    step-small sequence -- equal oracle.cpu_ref.GaussNewtonCGRef in float64 to 1e-12 over a (3, 4, 2) schedule, for all eight combinations of
    fletcher_reeves, standard_alpha and dff in {0, 0.5}.
(d) The discrimination condition of tests/test_solver_kernels_gpu.py's short solves: on their inputs, with dff = 0.5, flipping
    fletcher_reeves, standard_alpha or dff changes the float64 result by at least 1e-3 relative -- orders of magnitude above that test's gate,
    so a kernel that ignores a flag cannot pass it.
"""
import itertools
import os
import sys

import pytest
import torch

import _solver_refs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import cpu_ref as O  # noqa: E402

FLAGS = list(itertools.product((False, True), (False, True), (0.0, 0.5)))         # fletcher_reeves, standard_alpha, dff


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) operators
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_problem():
    """N = 3 samples, Cin = 12, c = 5, 6 x 7 maps, 96 x 112 labels (16x the map), hinge pixel weights, the memory's sample weights."""
    g = torch.Generator().manual_seed(11)
    N, Cin, c, h, w = 3, 12, 5, 6, 7
    Hh, Ww = 16 * h, 16 * w
    X = torch.relu(torch.randn(N, Cin, h, w, generator=g))
    Y = torch.zeros(N, 1, Hh, Ww)
    for k in range(N):
        Y[k, 0, 10 + 7 * k:40 + 5 * k, 20 + 3 * k:45 + 9 * k] = 1.0          # 7 to 9 % of the pixels: below tf
    pw = O.pixel_weights(Y, dict(method='hinge', tf=0.1))
    assert float(pw.min()) < float(pw.max())                       # the hinge rule really weights
    w1 = (torch.rand(c, Cin, 1, 1, generator=g) * 2 - 1) / Cin ** 0.5
    w2 = (torch.rand(1, c, 3, 3, generator=g) * 2 - 1) / (9 * c) ** 0.5
    p1 = torch.randn(c, Cin, 1, 1, generator=g) * 0.1
    p2 = torch.randn(1, c, 3, 3, generator=g) * 0.1
    B, cmap = O.lowres_normal(pw, Y, (h, w))
    return dict(N=N, Cin=Cin, c=c, h=h, w=w, X=X, Y=Y, pw=pw, w1=w1, w2=w2, p1=p1, p2=p2, B=B, cmap=cmap)


def _flat(c, Cin, t1, t2):
    """[projection part transposed to (Cin, c) | filter part] of a reference-layout pair."""
    return torch.cat([t1.reshape(c, Cin).t().reshape(-1), t2.reshape(-1)])


def test_joint_operator_equals_the_hires_reference(small_problem):
    d = small_problem
    N, Cin, c = d['N'], d['Cin'], d['c']
    mem = O.MemoryRef(N, d['X'].shape[1:], d['Y'].shape[1:], 0.1)
    mem.initialize(d['X'], d['Y'], d['pw'])
    reg = (1e-2, 3e-2)
    pr = O.InitProblemRef(mem, reg, (1.0, 1.0))
    pr.initialize()
    b_ref = pr.linearize([d['w1'], d['w2']])
    a_ref = pr.A([d['p1'], d['p2']])
    sw = mem.weights[:N]
    assert float(sw.min()) != float(sw.max())
    w1T, w2 = d['w1'].reshape(c, Cin).t().contiguous(), d['w2'].reshape(c, 9)
    lam1, lam2 = reg[0] ** 2, reg[1] ** 2
    b = S.joint_rhs(d['X'], w1T, w2, d['B'], d['cmap'], sw, lam1, lam2)
    a = S.joint_A(d['X'], w1T, w2, d['B'], sw, lam1, lam2, d['p1'].reshape(c, Cin).t().contiguous(), d['p2'].reshape(c, 9))
    eb, ea = _rel(b, _flat(c, Cin, *b_ref)), _rel(a, _flat(c, Cin, *a_ref))
    print('joint: b %.2e  A p %.2e' % (eb, ea))
    assert eb < 1e-5 and ea < 1e-5
    n1 = Cin * c                                                    # ... and each part on its own scale
    for lo, hi in ((0, n1), (n1, n1 + 9 * c)):
        assert _rel(b[lo:hi], _flat(c, Cin, *b_ref)[lo:hi]) < 1e-5 and _rel(a[lo:hi], _flat(c, Cin, *a_ref)[lo:hi]) < 1e-5


def test_filter_operator_equals_the_hires_reference(small_problem):
    d = small_problem
    N, Cin, c = d['N'], d['Cin'], d['c']
    Z = O.conv1x1(d['X'], d['w1'])
    mem = O.MemoryRef(N + 2, Z.shape[1:], d['Y'].shape[1:], 0.1)
    mem.initialize(Z, d['Y'], d['pw'])
    pr = O.UpdateProblemRef(mem, 3e-2, 1.0)
    pr.initialize()
    b_ref = pr.linearize([d['w2']])[0]
    a_ref = pr.A([d['p2']])[0]
    sw = mem.weights[:N]
    b = S.filter_rhs(Z, d['w2'].reshape(c, 9), d['B'], d['cmap'], sw, 3e-2 ** 2)
    a = S.filter_A(Z, d['p2'].reshape(c, 9), d['B'], sw, 3e-2 ** 2)
    eb, ea = _rel(b, b_ref.reshape(-1)), _rel(a, a_ref.reshape(-1))
    print('filter: b %.2e  A p %.2e' % (eb, ea))
    assert eb < 1e-5 and ea < 1e-5


def test_operator_pieces_compose_to_the_operators(small_problem):
    """The per-entry-point functions, chained the way the three joint forms chain the launches, give joint_A (float64, 1e-12)."""
    d = small_problem
    N, Cin, c, h, w = d['N'], d['Cin'], d['c'], d['h'], d['w']
    D = lambda t: t.double()
    X, B, sw = D(d['X']), D(d['B']), torch.tensor([0.5, 0.3, 0.2], dtype=torch.float64)
    w1T, w2 = D(d['w1']).reshape(c, Cin).t().contiguous(), D(d['w2']).reshape(c, 9)
    p1, p2 = D(d['p1']).reshape(c, Cin).t().contiguous(), D(d['p2']).reshape(c, 9)
    lam1, lam2 = 1e-4, 9e-4
    want = S.joint_A(X, w1T, w2, B, sw, lam1, lam2, p1, p2)
    Z = S.conv1x1(X, w1T)
    # fused form: scores2 -> joint_mid -> GEMM -> joint_q_pq
    s = S.filter_scores2(S.conv1x1(X, p1), w2, Z, p2)
    slabs, Dm = S.joint_mid(s, B, None, sw, Z, w2)
    g1 = torch.einsum('nip,npc->ic', X.reshape(N, Cin, h * w), Dm).reshape(-1)
    q = S.joint_q_pq(g1, lam1, slabs, N, c * 9, c * 9, lam2, p1.reshape(-1), p2.reshape(-1), 1.0)
    assert _rel(q, want) < 1e-12
    # composed form: compose -> scores_composed -> stencil_sum -> two weight gradients -> joint_q_pq_composed
    K = S.joint_compose(p1, w2)
    sp = S.joint_scores_composed(X, K, Z, p2, 5)
    assert sp.shape == (6, N, h * w)
    t = S.stencil_sum(B, None, sw, sp, h, w)
    assert _rel(t, S.stencil(B, None, sw, s)) < 1e-12
    GX, GZ = S.filter_wgrad(X, t), S.filter_wgrad(Z, t)
    q = S.joint_q_pq_composed(GX.reshape(N, Cin, 9), w2, lam1, GZ, N, c * 9, c * 9, lam2, p1, p2.reshape(-1), 1.0)
    assert _rel(q, want) < 1e-12
    assert _rel(S.joint_expand(GX.reshape(N, Cin, 9), w2, lam1, p1, -1.0).reshape(-1), -want[:Cin * c]) < 1e-12
    assert _rel(S.vec_reduce_slabs(GZ, N, c * 9, c * 9, lam2, p2.reshape(-1), -1.0), -want[Cin * c:]) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) adjoint pairs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_adjoint_pairs_float64():
    g = torch.Generator().manual_seed(5)
    N, C, h, w = 2, 4, 5, 9
    X = torch.randn(N, C, h, w, generator=g, dtype=torch.float64)
    f = torch.randn(C, 9, generator=g, dtype=torch.float64)
    t = torch.randn(N, h, w, generator=g, dtype=torch.float64)
    lhs = float((S.conv3x3(X, f) * t).sum())
    wg = float((S.filter_wgrad(X, t).sum(0) * f.reshape(-1)).sum())
    ig = float((S.filter_igrad(t, f) * X.reshape(N, C, h * w).transpose(1, 2)).sum())
    assert abs(lhs - wg) <= 1e-12 * abs(lhs) and abs(lhs - ig) <= 1e-12 * abs(lhs)
    # the stencil is its own transpose when B couples (i,j) with (i+di,j+dj) symmetrically; here only linearity in s and the zero border
    B = torch.randn(N, 9, h, w, generator=g, dtype=torch.float64)
    sw = torch.rand(N, generator=g, dtype=torch.float64)
    one = torch.zeros(N, h, w, dtype=torch.float64)
    one[:, 0, 0] = 1.0
    t1 = S.stencil(B, None, sw, one)
    assert torch.equal(t1[:, 0, 0], sw * B[:, 4, 0, 0]) and torch.equal(t1[:, 1, 1], sw * B[:, 0, 1, 1]) and float(t1[:, 2:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) CG transitions against GaussNewtonCGRef
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def dense():
    """Per layout: A0 and the right-hand sides (fp32 values) and the float64 GaussNewtonCGRef result for every flag set."""
    out = {}
    for name, layout in S.SOLVE_LAYOUTS.items():
        A0, rhs = S.spd_problem(layout[0] + layout[1], 7 + len(name))
        out[name] = (layout, A0, rhs, {fl: S.dense_reference(O, A0, rhs, layout, *fl, torch.float64) for fl in FLAGS})
    return out


@pytest.mark.parametrize('fr,sa,dff', FLAGS)
@pytest.mark.parametrize('name,form', [('small', 'small'), ('small', 'multi'), ('multi', 'multi')])
def test_cg_transitions_equal_the_reference_solver(dense, name, form, fr, sa, dff):
    (n1, n2, m1, m2), A0, rhs, refs = dense[name]
    A0, rhs = A0.double(), [b.double() for b in rhs]
    chain = S.CGChain(n1, n2, m1, m2, fr, sa, dff)
    x = torch.zeros(n1 + n2, dtype=torch.float64)
    step = 1.0
    for k, it in enumerate(S.SOLVE_SCHEDULE):
        if form == 'multi':
            dx = chain.run_multi(rhs[k], lambda p: A0 @ p + S.SOLVE_LAM * p, it)
        else:
            # three slabs 3 floats further apart than they are long, as a caller's slab buffer may be
            def slabs_of(p):
                q0 = A0 @ p
                buf = torch.zeros(3, n1 + 3, dtype=torch.float64)
                buf[0, :n1], buf[1, :n1], buf[2, :n1] = 0.5 * q0, 0.25 * q0, 0.25 * q0
                return buf, 3, n1 + 3, S.SOLVE_LAM
            dx = chain.run_small(rhs[k], slabs_of, it)
        x = x + step * dx
        step = min(step * 1.2, 1.0)
        e = _rel(x, refs[(fr, sa, dff)][k])
        assert e <= 1e-12, (name, form, fr, sa, dff, k, e)


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) the short solves tell the flags apart
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(S.SOLVE_LAYOUTS))
def test_the_short_solves_discriminate_every_flag(dense, name):
    _, _, _, refs = dense[name]
    for fr, sa in itertools.product((False, True), (False, True)):
        base = refs[(fr, sa, 0.5)][-1]
        flips = {'fletcher_reeves': refs[(not fr, sa, 0.5)][-1], 'standard_alpha': refs[(fr, not sa, 0.5)][-1], 'dff': refs[(fr, sa, 0.0)][-1]}
        for what, other in flips.items():
            d = _rel(other, base)
            print('%s fr %d sa %d: flipping %s changes the result by %.2e' % (name, fr, sa, what, d))
            assert d >= 1e-3, (name, fr, sa, what, d)
    # with dff = 0 the variants of exact CG on a linear problem coincide up to rounding: the regime in which a flag test means nothing
    assert _rel(refs[(True, True, 0.0)][-1], refs[(False, True, 0.0)][-1]) < 1e-9
