"""Every kernel of the chain form of the target-model solver (csrc/joint_fit.hip; the CG and stencil part of csrc/target_model.hip) against
its float64 definition (tests/_solver_refs.py, pinned by tests/test_solver_refs.py), called through the C entry points at the shapes the
kernels branch on: channel tails of the wave split, row-block and column-tile tails, empty channel groups and empty pixel parts, the
grid-stride second trips, the switch between the stencil-sum kernels, the LDS tiles above 64 KB, every CG flag.

Gate: the project's rule, tests/test_refiner_train_gpu.py::_gate,
    max|hip - ref64| <= max(4 * max|torch32 - ref64|, 1e-6 * max|ref64|)
with ref64 the reference in float64 on the CPU and torch32 the same expression in fp32 on the GPU.  Inputs are fp32 values from a seeded CPU
generator; all three legs read exactly those values.  Dot-product partials: the checked quantity is the float64 sum of the FRTM_CG_BLOCKS
block partials against the float64 dot, with the floor 1e-6 * sum|terms| (rounding there scales with the sum of magnitudes, not with a result
that may cancel).

Output hygiene: every output and every partials buffer is pre-filled with NaN and sits between two guard bands of 64 floats, which must stay
NaN; a NaN left in an output means "not written".  This holds for all 2 x 64 words of a bank and for the partial score maps of empty channel
groups.  Words a launch must not write are compared bit for bit.

Sections: 3a the operator kernels and their refusals; 3b the five CG kernels, one launch each, state in to state out; 3c short solves through
GaussNewtonCG.run on a dense problem, every CG flag, against oracle.cpu_ref.GaussNewtonCGRef in float64 (tests/test_solver_refs.py asserts
that these inputs tell the flags apart by 1e-3 or more); 3d the three joint forms and the filter form of DiscriminatorLoss off the fixture
shapes, B, c, sw and the features read back from the memory object.

frtm_cg_step_small forms its dot products inside the launch, so its outputs carry their rounding; for this kernel the bound gains a derived
term, passed as the gate's floor.  Derivation: grant every dot of the launch what the partials above are granted, D(t) = 1e-6 * sum|t_i|, and
propagate to first order.  With N = rho (standard_alpha, an input: dN = 0) or N = <p,r> (dN = D(p r)):
    alpha = N / <p,q>:            d_alpha = (dN + |alpha| D(p q)) / |<p,q>|                     state[1]
    x (+)= alpha p:               max|p| d_alpha
    rn = r - alpha q:             max|q| d_alpha
    rho' = <rn,z>, z = rn / M:    d_rho' = D(rn z) + (2 / M) |<q,rn>| d_alpha                   state[4]
    rho2 = <r,z>:                 d_rho2 = D(r z) + (1 / M) |<r,q>| d_alpha
    beta = (rho' [- rho2]) / rho: d_beta = (d_rho' [+ d_rho2]) / |rho|                          state[2]
    p = z + beta p:               (1 / M) max|q| d_alpha + max|p| d_beta
(all from the float64 operands; _step_small_floors).  The term matters for beta and p: with independent draws rho' and rho2 are two numbers
near 4000 whose difference, a few units, is divided by a rho near 1 -- rounding rho' and rho2 to fp32 alone moves beta by 5e-4, and the fp32
reference on the CPU shows the same error as the kernel (p at n = 1024: 1.53e-3 both), while the fp32 leg on the GPU happened to land 460
times closer.  Without the term the kernel measured up to 461 x the yardstick on p and 2.4 x on beta; no other output needed it.

No test here asserts a time.  The module (464 tests) ran in 10 to 11.5 s on an MI355X (14 s wall with the interpreter's start).  Largest RATIO
(hip error / torch32 error) per kernel over two runs (the fp32 leg's own error moves a little from run to run); ratios above 4 passed on
the 1e-6 floors (of max|ref|, or of sum|terms| for dots):
    k_scores2_rows 2.27   k_filter_scores_rows (split) 6.10   k_stencil_sum 1.00   k_stencil (summed maps) 4.65   k_scores_composed 4.14
    k_joint_compose 1.27   k_joint_expand 1.99   k_joint_mid 3.73 (68 x 120: 0.60)   k_vec_reduce_slabs 1.00   k_vec_axpy 1.00
    k_joint_q_pq 1.58 on q, 102 on a dot   k_joint_q_pq_c 1.62 on q, 23.5 on a dot   k_cg_begin 2.38   k_cg_pq 13.0 (n = 5)
    k_cg_direction 22.3 (rho_new, the 64 partials added one after the other)   k_cg_update 14.5 (alpha)   k_cg_step_small 461 (p, see above)
    short solves: step-small path 0.52, multi-kernel path 0.98 -- inside the plain yardstick (one fp32 run of the reference), which is
    therefore not widened by further draws
    DiscriminatorLoss: joint linearize 2.57, apply_A 0.89, apply_A_pq 0.89 on q and 21.8 on a dot; filter linearize 0.81, apply_A 0.76
"""
import itertools
import math
import os
import sys

import pytest
import torch

import _solver_refs as S
from test_refiner_train_gpu import _gate

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
NAN = float('nan')
BLOCKS = S.CG_BLOCKS
DOT_EPS = 1e-6          # the floor of a dot product, per unit of sum|terms|


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _uniform(g, lo, hi, *shape):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Buf:
    """A device buffer of `shape` between two NaN guard bands: NaN-filled (an output) or holding `init` (fp32 values from the CPU)."""

    def __init__(self, *shape, init=None):
        if init is not None:
            shape = tuple(init.shape)
        n = int(math.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), NAN, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(init)
        self.before = self.t.clone()
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0

    def guards(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:GUARD]).all()), 'write below the buffer'
        assert bool(torch.isnan(self.buf[GUARD + self.t.numel():]).all()), 'write above the buffer'

    def done(self):
        """The guards are untouched and every element was written; returns the buffer."""
        self.guards()
        assert not bool(torch.isnan(self.t).any()), 'output element not written'
        return self.t

    def same(self):
        """The guards and every word are what they were before the launch, bit for bit."""
        self.guards()
        assert torch.equal(_bits(self.t), _bits(self.before)), 'a word that the launch must not write has changed'
        return self.t


def _check(kernel, case, hip, ref64, t32, floor=None):
    """The gate, with the figures printed first (`pytest -s` shows them): hip error, torch32 error, their ratio."""
    e = float((hip.double().cpu() - ref64.double().cpu()).abs().max())
    e32 = float((t32.double().cpu() - ref64.double().cpu()).abs().max())
    print('RATIO %s %s hip %.3e torch32 %.3e ratio %.3f max|ref| %.3e' % (kernel, case, e, e32, e / max(e32, 1e-30) if e else 0.0,
                                                                            float(ref64.abs().max()) if ref64.numel() else 0.0))
    assert tuple(hip.shape) == tuple(ref64.shape)
    _gate(hip, ref64, t32, '%s %s' % (kernel, case), floor=floor)


def _check_dot(kernel, case, words, terms64, terms32):
    """`words`: the FRTM_CG_BLOCKS partials of one dot product; their float64 sum against the float64 dot, floor 1e-6 * sum|terms|."""
    assert words.numel() == BLOCKS and not bool(torch.isnan(words).any())
    _check(kernel, case, words.double().sum().reshape(1), terms64.sum().reshape(1), terms32.sum().reshape(1),
           floor=DOT_EPS * float(terms64.abs().sum()))


def _legs(fn, *args):
    """fn on the float64 copies of the (fp32, CPU) arguments on the CPU, and on their fp32 copies on the GPU."""
    def to(a, f):
        return f(a) if torch.is_tensor(a) else a
    return fn(*[to(a, lambda t: t.double()) for a in args]), fn(*[to(a, lambda t: t.to(DEV)) for a in args])


def _call(name, *args):
    from frtm_vos_amd import _hip as H
    H.call(name, *[H.ptr(a) if torch.is_tensor(a) else a for a in args])


def _d(t):
    return None if t is None else t.to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3a. operator kernels
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [5, 16, 17, 40])
@pytest.mark.parametrize('h,w', [(1, 1), (4, 63), (7, 64), (5, 65)])
def test_filter_scores2(C, h, w):
    """16 waves split C (tails: C = 5, 17, 40), 3 rows per block (h = 1, 4, 7), lane = column; w = 65 takes the two-launch fallback."""
    N = 2
    g = _gen(C, h, w, 1)
    X1, X2, f1, f2 = _randn(g, N, C, h, w), _randn(g, N, C, h, w), _randn(g, C, 9) * 0.3, _randn(g, C, 9) * 0.3
    out = _Buf(N, h, w)
    _call('frtm_filter_scores2', _d(X1), _d(f1), _d(X2), _d(f2), N, C, h, w, out.t)
    r64, r32 = _legs(S.filter_scores2, X1, f1, X2, f2)
    _check('k_scores2_rows', 'C%d %dx%d' % (C, h, w), out.done(), r64, r32)


def _stencil_inputs(g, N, h, w, with_c):
    B, sw = _randn(g, N, 9, h, w), _uniform(g, 0.1, 1.0, N)
    return B, (_randn(g, N, h, w) if with_c else None), sw


@pytest.mark.parametrize('splits', [1, 3, 8, 9, 64])
@pytest.mark.parametrize('C', [2, 10, 100])
@pytest.mark.parametrize('h', [1, 4, 9])
@pytest.mark.parametrize('w', [3, 64])
def test_filter_scores_split_and_stencil_sum(splits, C, h, w):
    """Partial score maps per channel group (groups with no channel give zero maps, which must be written), then frtm_stencil_sum over them,
    with and without c: 8 maps against 9 is the switch from the one-block to the row-block kernel."""
    N = 2
    g = _gen(splits, C, h, w, 2)
    X, f = _randn(g, N, C, h, w), _randn(g, C, 9) * 0.3
    part = _Buf(splits, N, h * w)
    _call('frtm_filter_scores_split', _d(X), _d(f), N, C, h, w, splits, part.t)
    r64, r32 = _legs(lambda a, b: S.filter_scores_split(a, b, splits), X, f)
    maps = part.done()
    _check('k_filter_scores_rows(split)', 'splits %d C%d %dx%d' % (splits, C, h, w), maps, r64, r32)
    _check('k_filter_scores_rows(split)', 'sum of the maps, splits %d C%d %dx%d' % (splits, C, h, w), maps.double().sum(0), r64.sum(0), r32.sum(0))
    maps_cpu = maps.cpu()
    for with_c in (False, True):
        B, c, sw = _stencil_inputs(g, N, h, w, with_c)
        t = _Buf(N, h, w)
        _call('frtm_stencil_sum', _d(B), _d(c), _d(sw), maps, splits, N, h, w, t.t)
        t64, t32 = _legs(lambda B_, c_, sw_, m_: S.stencil_sum(B_, c_, sw_, m_, h, w), B, c, sw, maps_cpu)
        _check('k_stencil_sum', 'nsum %d %dx%d c %d' % (splits, h, w, with_c), t.done(), t64, t32)
        # ... and frtm_stencil over the torch-summed maps
        t2 = _Buf(N, h, w)
        _call('frtm_stencil', _d(B), _d(c), _d(sw), maps.sum(0).contiguous(), N, h, w, t2.t)
        _check('k_stencil', 'over the summed maps, nsum %d %dx%d c %d' % (splits, h, w, with_c), t2.done(), t64, t32)
    part.guards()


@pytest.mark.parametrize('nsum,h,w', [(3, 130, 130), (8, 130, 130), (9, 130, 130), (9, 9, 130), (2, 126, 126)])
def test_stencil_sum_large_maps(nsum, h, w):
    """130 x 130: the padded map is above 64 KB of LDS, so up to 8 maps take the third path (frtm_stencil's kernel summing the maps itself), 9
    the row-block kernel; 126 x 126 is the largest tile of the one-block kernel (64 KB exactly)."""
    N = 2
    g = _gen(nsum, h, w, 3)
    assert ((h + 2) * (w + 2) * 4 > 65536) == (h == 130)
    maps = _randn(g, nsum, N, h * w)
    B, c, sw = _stencil_inputs(g, N, h, w, True)
    t = _Buf(N, h, w)
    _call('frtm_stencil_sum', _d(B), _d(c), _d(sw), _d(maps), nsum, N, h, w, t.t)
    t64, t32 = _legs(lambda B_, c_, sw_, m_: S.stencil_sum(B_, c_, sw_, m_, h, w), B, c, sw, maps)
    _check('k_stencil_sum', 'nsum %d %dx%d' % (nsum, h, w), t.done(), t64, t32)


@pytest.mark.parametrize('Cx,splits', [(10, 3), (100, 1), (3, 8), (64, 64)])
@pytest.mark.parametrize('Cz', [1, 17])
@pytest.mark.parametrize('h,w', [(2, 5), (7, 64), (4, 65), (3, 129)])
def test_joint_scores_composed(Cx, splits, Cz, h, w):
    """Narrow maps and the column-tile seam (65 and 129 columns: two and three tiles, the neighbours across a seam loaded); (100, 1): 7 channels
    per wave, a tail of the 4-channel trips; (3, 8): empty groups."""
    N = 2
    g = _gen(Cx, splits, Cz, h, w, 4)
    X, K, Z, p2 = _randn(g, N, Cx, h, w), _randn(g, Cx, 9) * 0.3, _randn(g, N, Cz, h, w), _randn(g, Cz, 9) * 0.3
    part = _Buf(splits + 1, N, h * w)
    _call('frtm_joint_scores_composed', _d(X), _d(K), Cx, _d(Z), _d(p2), Cz, N, h, w, splits, part.t)
    r64, r32 = _legs(lambda a, b, c, d: S.joint_scores_composed(a, b, c, d, splits), X, K, Z, p2)
    _check('k_scores_composed', 'Cx%d/%d Cz%d %dx%d' % (Cx, splits, Cz, h, w), part.done(), r64, r32)


@pytest.mark.parametrize('Cin', [1, 5, 64])
@pytest.mark.parametrize('c', [1, 63, 64, 65, 128])
def test_joint_compose(Cin, c):
    g = _gen(Cin, c, 5)
    p1, w2 = _randn(g, Cin, c), _randn(g, c, 9) * 0.3
    K = _Buf(Cin, 9)
    _call('frtm_joint_compose', _d(p1), _d(w2), Cin, c, K.t)
    r64, r32 = _legs(S.joint_compose, p1, w2)
    _check('k_joint_compose', 'Cin%d c%d' % (Cin, c), K.done(), r64, r32)


@pytest.mark.parametrize('Cin', [3, 8])
@pytest.mark.parametrize('c', [7, 65, 128])
@pytest.mark.parametrize('nslab', [1, 5])
@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_joint_expand(Cin, c, nslab, sign):
    """4 c > 256 (c = 65, 128) forces a second trip of the output loop; Cin = 3: a block with a missing channel."""
    g = _gen(Cin, c, nslab, 6)
    G, w2, p1 = _randn(g, nslab, Cin, 9), _randn(g, c, 9) * 0.3, _randn(g, Cin, c)
    q1 = _Buf(Cin, c)
    _call('frtm_joint_expand', _d(G), nslab, _d(w2), Cin, c, 0.37, _d(p1), sign, q1.t)
    r64, r32 = _legs(lambda a, b, d: S.joint_expand(a, b, 0.37, d, sign), G, w2, p1)
    _check('k_joint_expand', 'Cin%d c%d nslab %d sign %+d' % (Cin, c, nslab, sign), q1.done(), r64, r32)


def _joint_mid_case(N, C, parts, h, w, with_cm):
    g = _gen(N, C, parts, h, w, with_cm, 7)
    s, Z, w2 = _randn(g, N, h, w), _randn(g, N, C, h, w), _randn(g, C, 9) * 0.3
    B, cm, sw = _stencil_inputs(g, N, h, w, with_cm)
    partial, D = _Buf(N * parts, C * 9), _Buf(N, h * w, C)
    _call('frtm_joint_mid', _d(s), _d(B), _d(cm), _d(sw), _d(Z), _d(w2), N, C, h, w, parts, partial.t, D.t)
    (g64, D64), (g32, D32) = _legs(S.joint_mid, s, B, cm, sw, Z, w2)
    case = 'N%d C%d parts %d %dx%d cm %d' % (N, C, parts, h, w, with_cm)
    _check('k_joint_mid', 'slabs ' + case, partial.done().double().view(N, parts, C * 9).sum(1), g64, g32)
    _check('k_joint_mid', 'D ' + case, D.done(), D64, D32)


@pytest.mark.parametrize('C', [1, 5, 18, 40])
@pytest.mark.parametrize('parts', [1, 3, 8, 64])
@pytest.mark.parametrize('h,w', [(3, 3), (17, 31), (30, 60)])
@pytest.mark.parametrize('with_cm', [False, True])
def test_joint_mid(C, parts, h, w, with_cm):
    """Channel tails of the 4 x 4-channel blocks; parts > h w / 64 gives empty parts (zero slabs, which must be written); C = 40 at 30 x 60:
    C h w > 64 * 1024, so the input-gradient blocks take a second grid-stride trip."""
    _joint_mid_case(2, C, parts, h, w, with_cm)


def test_joint_mid_lds_above_64k():
    """68 x 120 (1080p): the two padded maps take 68 KB of LDS, the path that raises the kernel's dynamic LDS limit."""
    assert 2 * 70 * 122 * 4 > 64 * 1024
    _joint_mid_case(1, 5, 5, 68, 120, True)


def _slab_buffer(g, nslab, stride, n):
    """(nslab, stride) slabs of n floats each; the stride - n floats between two slabs are NaN: reading one poisons the output."""
    buf = torch.full((nslab, max(stride, n)), NAN)
    buf[:, :n] = _randn(g, nslab, n)
    return buf


def _q_variants():
    """(sign, r given, partial given)"""
    return list(itertools.product((1.0, -1.0), (False, True), (False, True)))


def _check_q_and_partials(kernel, case, q, partial, q64, q32, p, r):
    _check(kernel, 'q ' + case, q.done(), q64, q32)
    if partial is None:
        return
    partial.guards()
    words = partial.t.view(2, BLOCKS, 2)
    assert bool(torch.isnan(words[1]).all()), 'the second bank was written'
    assert not bool(torch.isnan(words[0]).any()), 'a partial word of the bank was not written'
    _check_dot(kernel, '<p,q> ' + case, words[0, :, 0], S.dot_terms(p.double(), q64), S.dot_terms(_d(p), q32))
    if r is None:
        assert bool((words[0, :, 1] == 0).all())
    else:
        _check_dot(kernel, '<p,r> ' + case, words[0, :, 1], S.dot_terms(p.double(), r.double()), S.dot_terms(_d(p), _d(r)))


@pytest.mark.parametrize('n1,n2', [(7, 9), (300, 45), (98304, 864)])
@pytest.mark.parametrize('nslab', [1, 7, 8, 9, 40])
@pytest.mark.parametrize('pad', [0, 5])
def test_joint_q_pq(n1, n2, nslab, pad):
    """nslab 7 / 8 / 9 / 40: the tail, one full trip, a trip and a tail, five trips of the eight-accumulator slab loop; stride = n2 and n2 + 5;
    98304 + 864 elements: six grid-stride trips of the 64 blocks."""
    g = _gen(n1, n2, nslab, pad, 8)
    stride = n2 + pad
    g1, slabs, p1, p2, r = _randn(g, n1), _slab_buffer(g, nslab, stride, n2), _randn(g, n1), _randn(g, n2), _randn(g, n1 + n2)
    p = torch.cat([p1, p2])
    for sign, with_r, with_partial in _q_variants():
        q, partial = _Buf(n1 + n2), (_Buf(4 * BLOCKS) if with_partial else None)
        _call('frtm_joint_q_pq', _d(g1), n1, 0.25, _d(slabs), nslab, stride, n2, 0.6, _d(p1), _d(p2), sign, q.t, _d(r) if with_r else None,
              None if partial is None else partial.t)
        q64, q32 = _legs(lambda a, b, c, d: S.joint_q_pq(a, 0.25, b, nslab, stride, n2, 0.6, c, d, sign), g1, slabs, p1, p2)
        case = 'n %d+%d nslab %d stride %d sign %+d r %d' % (n1, n2, nslab, stride, sign, with_r)
        _check_q_and_partials('k_joint_q_pq', case, q, partial, q64, q32, p, r if with_r else None)


@pytest.mark.parametrize('Cin,c', [(1, 1), (70, 24), (1000, 96), (2048, 128)])
@pytest.mark.parametrize('nslabX', [1, 6])
@pytest.mark.parametrize('nslab', [1, 9])
def test_joint_q_pq_composed(Cin, c, nslabX, nslab):
    """(2048, 128): 32 channels per block, so both inner loops (288 slab sums, 4096 outputs over 256 threads) take further trips; (70, 24): two
    channels in the first 35 blocks, none in the rest; nslab 9 with stride = n2 + 5."""
    g = _gen(Cin, c, nslabX, nslab, 9)
    n1, n2 = Cin * c, c * 9
    stride = n2 + (5 if nslab == 9 else 0)
    GX, w2, slabs = _randn(g, nslabX, Cin, 9), _randn(g, c, 9) * 0.3, _slab_buffer(g, nslab, stride, n2)
    p1, p2, r = _randn(g, Cin, c), _randn(g, n2), _randn(g, n1 + n2)
    p = torch.cat([p1.reshape(-1), p2])
    for sign, with_r, with_partial in _q_variants():
        q, partial = _Buf(n1 + n2), (_Buf(4 * BLOCKS) if with_partial else None)
        _call('frtm_joint_q_pq_composed', _d(GX), nslabX, Cin, c, _d(w2), 0.25, _d(slabs), nslab, stride, n2, 0.6, _d(p1), _d(p2), sign, q.t,
              _d(r) if with_r else None, None if partial is None else partial.t)
        q64, q32 = _legs(lambda a, b, s_, d, e: S.joint_q_pq_composed(a, b, 0.25, s_, nslab, stride, n2, 0.6, d, e, sign), GX, w2, slabs, p1, p2)
        case = 'Cin%d c%d nslabX %d nslab %d sign %+d r %d' % (Cin, c, nslabX, nslab, sign, with_r)
        _check_q_and_partials('k_joint_q_pq_c', case, q, partial, q64, q32, p, r if with_r else None)


@pytest.mark.parametrize('n', [5, 131072 + 3])
@pytest.mark.parametrize('nslab,pad', [(1, None), (3, 0), (9, 5)])
@pytest.mark.parametrize('with_p', [False, True])
def test_vec_reduce_slabs(n, nslab, pad, with_p):
    """pad None: stride 0 with one slab, as DiscriminatorLoss._project_grad calls it; 131072 + 3 elements: the 512 blocks take a second trip."""
    g = _gen(n, nslab, with_p, 10)
    stride = 0 if pad is None else n + pad
    slabs, p = _slab_buffer(g, nslab, stride, n), (_randn(g, n) if with_p else None)
    for sign in (1.0, -1.0):
        q = _Buf(n)
        _call('frtm_vec_reduce_slabs', _d(slabs), nslab, stride, n, 0.6, _d(p), sign, q.t)
        q64, q32 = _legs(lambda a, b: S.vec_reduce_slabs(a, nslab, stride, n, 0.6, b, sign), slabs, p)
        _check('k_vec_reduce_slabs', 'n %d nslab %d stride %d p %d sign %+d' % (n, nslab, stride, with_p, sign), q.done(), q64, q32)


@pytest.mark.parametrize('n', [5, 98304])
def test_vec_axpy(n):
    g = _gen(n, 11)
    y0, x = _randn(g, n), _randn(g, n)
    y = _Buf(init=y0)
    _call('frtm_vec_axpy', y.t, 0.83, _d(x), n)
    r64, r32 = _legs(lambda a, b: S.vec_axpy(a, 0.83, b), y0, x)
    _check('k_vec_axpy', 'n %d' % n, y.done(), r64, r32)


# ---- refusals: each raises through H.call and leaves its NaN-filled outputs untouched
def _z(*shape):
    return torch.zeros(*shape, device=DEV)


def test_refusals():
    K = _Buf(2, 9)
    with pytest.raises(RuntimeError, match='frtm_joint_compose'):
        _call('frtm_joint_compose', _z(2, 129), _z(129, 9), 2, 129, K.t)
    K.same()
    for Cin, c in ((2, 129), (2049, 4)):
        q, partial = _Buf(Cin * c + 9 * c), _Buf(4 * BLOCKS)
        with pytest.raises(RuntimeError, match='frtm_joint_q_pq_composed'):
            _call('frtm_joint_q_pq_composed', _z(1, Cin, 9), 1, Cin, c, _z(c, 9), 0.1, _z(1, c * 9), 1, c * 9, c * 9, 0.1, _z(Cin, c), _z(c * 9), 1.0, q.t,
                  None, partial.t)
        q.same(), partial.same()
    part = _Buf(2, 2, 3 * 65)
    with pytest.raises(RuntimeError, match='frtm_filter_scores_split'):
        _call('frtm_filter_scores_split', _z(2, 4, 3, 65), _z(4, 9), 2, 4, 3, 65, 2, part.t)
    part.same()
    slabs, D = _Buf(2 * 65, 4 * 9), _Buf(2, 9, 4)
    with pytest.raises(RuntimeError, match='frtm_joint_mid'):
        _call('frtm_joint_mid', _z(2, 3, 3), _z(2, 9, 3, 3), None, _z(2), _z(2, 4, 3, 3), _z(4, 9), 2, 4, 3, 3, 65, slabs.t, D.t)
    slabs.same(), D.same()
    n = 1025
    vec = [_Buf(n) for _ in range(5)]
    state = _Buf(8)
    with pytest.raises(RuntimeError, match='frtm_cg_step_small'):
        _call('frtm_cg_step_small', _z(n), 1, n, 0.1, *[v.t for v in vec], n, 1.0, 1, 0, 1, 0, state.t)
    for v in vec + [state]:
        v.same()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3b. CG kernels, one launch each, state in to state out
# ---------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = [(5, 0), (864, 0), (1000, 37), (98304, 864)]
INV_M1, INV_M2 = 4.0, 0.25


def _cg_inputs(n, *key, rho2_scale=0.37):
    """Independent draws: five vectors, state[0..5] in (0.5, 1.5) (state[6..7] NaN: never read, never written), and a bank whose two column
    sums lie near 1 and near rho2_scale."""
    g = _gen(n, *key)
    v = {k: _randn(g, n) for k in ('x', 'r', 'r_prev', 'p', 'q')}
    state = torch.full((8,), NAN)
    state[:6] = _uniform(g, 0.5, 1.5, 6)
    bank = _uniform(g, 0.5, 1.5, BLOCKS, 2) / BLOCKS
    bank[:, 1] *= rho2_scale
    return v, state, bank


def _partial_with(bank, which):
    """The two banks of a partials buffer, bank `which` holding `bank`, the other one NaN."""
    both = torch.full((2, BLOCKS, 2), NAN)
    both[which] = bank
    return _Buf(init=both)


def _check_state(kernel, case, state, written, st64, st32, floors=None):
    """The state words in `written` against the transition; every other word bit for bit as before the launch."""
    state.guards()
    for k in written:
        assert not bool(torch.isnan(state.t[k]))
        _check(kernel, 'state[%d] %s' % (k, case), state.t[k:k + 1], st64[k:k + 1], st32[k:k + 1], floor=(floors or {}).get(k))
    rest = [k for k in range(8) if k not in written]
    assert torch.equal(_bits(state.t)[rest], _bits(state.before)[rest]), 'a state word that the launch must not write has changed'


def _check_bank(kernel, case, words, t64, t32):
    """words (BLOCKS, 2) written by the launch against the term vectors of its two dots (None: the word is an exact zero)."""
    assert not bool(torch.isnan(words).any()), 'a partial word of the bank was not written'
    for k in range(2):
        if t64[k] is None:
            assert bool((words[:, k] == 0).all())
        else:
            _check_dot(kernel, 'bank word %d %s' % (k, case), words[:, k], t64[k], t32[k])


def _z_terms(rn, rv, n1):
    z = rn * S._inv_m(rn, n1, INV_M1, INV_M2)
    return rn * z, rv * z


@pytest.mark.parametrize('n1,n2', LAYOUTS)
@pytest.mark.parametrize('has_p', [0, 1])
def test_cg_begin(n1, n2, has_p):
    n = n1 + n2
    v, _, _ = _cg_inputs(n, has_p, 20)
    r, partial = _Buf(n), _Buf(4 * BLOCKS)
    _call('frtm_cg_begin', _d(v['q']), r.t, _d(v['r_prev']) if has_p else None, n1, n2, INV_M1, INV_M2, has_p, partial.t)
    assert torch.equal(r.done().cpu(), v['q'])
    partial.guards()
    words = partial.t.view(2, BLOCKS, 2)
    assert bool(torch.isnan(words[0]).all()), 'the first bank was written'
    case = 'n %d+%d has_p %d' % (n1, n2, has_p)
    t64 = _z_terms(v['q'].double(), v['r_prev'].double(), n1)
    t32 = _z_terms(_d(v['q']), _d(v['r_prev']), n1)
    _check_bank('k_cg_begin', case, words[1], (t64[0], t64[1] if has_p else None), t32)
    (r64, b64), _ = _legs(lambda b_, rp_: S.cg_begin(b_, rp_, n1, INV_M1, INV_M2, has_p), v['q'], v['r_prev'])
    assert torch.equal(r64, v['q'].double())
    assert abs(float(b64[:, 0].sum() - t64[0].sum())) <= 1e-12 * float(t64[0].abs().sum())          # the transition's bank is these dots


@pytest.mark.parametrize('n1,n2', LAYOUTS)
@pytest.mark.parametrize('has_p,apply_dff,fr,clamp', [(h_, a_, f_, False) for h_, a_, f_ in itertools.product((0, 1), repeat=3)] + [(1, 1, 0, True)])
def test_cg_direction(n1, n2, has_p, apply_dff, fr, clamp):
    """dff = 0.5.  clamp: rho_new < rho2, so the Polak-Ribiere beta is negative and the clamp to 0 binds.  has_p = 0: p holds NaN on entry
    (it is written, never read)."""
    n = n1 + n2
    v, st, bank = _cg_inputs(n, has_p, apply_dff, fr, clamp, 21, rho2_scale=3.0 if clamp else 0.37)
    p0 = v['p'] if has_p else torch.full((n,), NAN)
    p, state, partial = _Buf(init=p0), _Buf(init=st), _partial_with(bank, 1)
    _call('frtm_cg_direction', _d(v['r']), p.t, n1, n2, INV_M1, INV_M2, has_p, apply_dff, fr, 0.5, state.t, partial.t)
    (p64, st64), (p32, st32) = _legs(lambda r_, p_, s_, b_: S.cg_direction(r_, p_, n1, INV_M1, INV_M2, has_p, apply_dff, fr, 0.5, s_, b_), v['r'], p0, st,
                                     bank)
    case = 'n %d+%d has_p %d dff %d fr %d clamp %d' % (n1, n2, has_p, apply_dff, fr, clamp)
    if clamp:
        assert float(st64[2]) == 0.0 and float(state.t[2]) == 0.0
    elif has_p:
        assert float(st64[2]) > 0.1
    _check('k_cg_direction', 'p ' + case, p.done(), p64, p32)
    _check_state('k_cg_direction', case, state, (2, 4), st64, st32)
    partial.same()


@pytest.mark.parametrize('n1,n2', LAYOUTS)
@pytest.mark.parametrize('with_r', [False, True])
def test_cg_pq(n1, n2, with_r):
    n = n1 + n2
    v, _, _ = _cg_inputs(n, with_r, 22)
    partial = _Buf(4 * BLOCKS)
    _call('frtm_cg_pq', _d(v['p']), _d(v['q']), _d(v['r']) if with_r else None, n, partial.t)
    partial.guards()
    words = partial.t.view(2, BLOCKS, 2)
    assert bool(torch.isnan(words[1]).all()), 'the second bank was written'
    t64 = (v['p'].double() * v['q'].double(), v['p'].double() * v['r'].double() if with_r else None)
    t32 = (_d(v['p']) * _d(v['q']), _d(v['p']) * _d(v['r']))
    _check_bank('k_cg_pq', 'n %d r %d' % (n, with_r), words[0], t64, t32)


@pytest.mark.parametrize('n1,n2', LAYOUTS)
@pytest.mark.parametrize('first,last,std', list(itertools.product((0, 1), repeat=3)))
def test_cg_update(n1, n2, first, last, std):
    """first: x holds NaN on entry (written, not read).  r_prev always holds NaN on entry.  last: r stays, bit for bit."""
    n = n1 + n2
    v, st, bank = _cg_inputs(n, first, last, std, 23)
    x0 = torch.full((n,), NAN) if first else v['x']
    x, r, r_prev, state, partial = _Buf(init=x0), _Buf(init=v['r']), _Buf(n), _Buf(init=st), _partial_with(bank, 0)
    _call('frtm_cg_update', x.t, r.t, r_prev.t, _d(v['p']), _d(v['q']), n1, n2, INV_M1, INV_M2, first, last, std, state.t, partial.t)
    legs = _legs(lambda x_, r_, p_, q_, s_, b_: S.cg_update(x_, r_, None, p_, q_, n1, INV_M1, INV_M2, first, last, std, s_, b_), x0, v['r'], v['p'],
                 v['q'], st, bank)
    (x64, r64, rp64, st64, _), (x32, r32, rp32, st32, _) = legs
    case = 'n %d+%d first %d last %d std %d' % (n1, n2, first, last, std)
    _check('k_cg_update', 'x ' + case, x.done(), x64, x32)
    if last:
        r.same()
    else:
        _check('k_cg_update', 'r ' + case, r.done(), r64, r32)
    assert torch.equal(r_prev.done().cpu(), v['r'])
    _check_state('k_cg_update', case, state, (0, 1), st64, st32)
    assert torch.equal(_bits(state.t[0:1]), _bits(state.before[4:5]))                 # rho <- rho_new, a copy
    partial.guards()
    words = partial.t.view(2, BLOCKS, 2)
    assert torch.equal(_bits(words[0]), _bits(partial.before.view(2, BLOCKS, 2)[0])), 'the bank the launch reads has changed'
    rn_hip = r.t.cpu()                                               # the dots are over the r the launch left (given to all legs)
    _check_bank('k_cg_update', case, words[1], _z_terms(rn_hip.double(), v['r'].double(), n1), _z_terms(_d(rn_hip), _d(v['r']), n1))


def _step_small_floors(p, q, r, rho, invM, last, std, fr):
    """The derived floor terms of frtm_cg_step_small's outputs (module docstring), from the float64 operands: {'x', 'r', 'p', 1, 2, 4}."""
    D = lambda t: DOT_EPS * float(t.abs().sum())
    amax = lambda t: float(t.abs().max())
    pq = float((p * q).sum())
    alpha = (rho if std else float((p * r).sum())) / pq
    d_alpha = ((0.0 if std else D(p * r)) + abs(alpha) * D(p * q)) / abs(pq)
    fl = {'x': amax(p) * d_alpha, 'r': amax(q) * d_alpha, 1: d_alpha}
    if not last:
        rn = r - alpha * q
        z = invM * rn
        d_s1 = D(rn * z) + 2 * invM * abs(float((q * rn).sum())) * d_alpha
        d_s2 = D(r * z) + invM * abs(float((r * q).sum())) * d_alpha
        d_beta = (d_s1 + (0.0 if fr else d_s2)) / abs(rho)
        fl.update({4: d_s1, 2: d_beta, 'p': invM * amax(q) * d_alpha + amax(p) * d_beta})
    return fl


@pytest.mark.parametrize('n', [5, 864, 1024])
@pytest.mark.parametrize('nslab', [1, 8, 9, 40])
def test_cg_step_small(n, nslab):
    """first x last x standard_alpha x fletcher_reeves.  x (first), r_prev and q hold NaN on entry; on `last` r, p, state[4] and state[2] stay,
    bit for bit, and state[0] receives the run's last rho."""
    for first, last, std, fr in itertools.product((0, 1), repeat=4):
        v, st, _ = _cg_inputs(n, nslab, first, last, std, fr, 24)
        g = _gen(n, nslab, 25)
        stride = n + 3
        slabs = _slab_buffer(g, nslab, stride, n)
        slabs[:, :n] /= nslab ** 0.5
        x0 = torch.full((n,), NAN) if first else v['x']
        x, r, r_prev, p, q, state = _Buf(init=x0), _Buf(init=v['r']), _Buf(n), _Buf(init=v['p']), _Buf(n), _Buf(init=st)
        _call('frtm_cg_step_small', _d(slabs), nslab, stride, 0.6, x.t, r.t, r_prev.t, p.t, q.t, n, INV_M1, first, last, std, fr, state.t)
        legs = _legs(lambda sl_, x_, r_, p_, s_: S.cg_step_small(sl_, nslab, stride, 0.6, x_, r_, None, p_, n, INV_M1, first, last, std, fr, s_),
                     slabs, x0, v['r'], v['p'], st)
        (x64, r64, rp64, p64, q64, st64), (x32, r32, rp32, p32, q32, st32) = legs
        case = 'n %d nslab %d first %d last %d std %d fr %d' % (n, nslab, first, last, std, fr)
        fl = _step_small_floors(v['p'].double(), q64, v['r'].double(), float(st[4]), INV_M1, last, std, fr)
        _check('k_cg_step_small', 'q ' + case, q.done(), q64, q32)
        _check('k_cg_step_small', 'x ' + case, x.done(), x64, x32, floor=fl['x'])
        assert torch.equal(r_prev.done().cpu(), v['r'])
        if last:
            r.same(), p.same()
            _check_state('k_cg_step_small', case, state, (0, 1), st64, st32, floors=fl)
        else:
            _check('k_cg_step_small', 'r ' + case, r.done(), r64, r32, floor=fl['r'])
            _check('k_cg_step_small', 'p ' + case, p.done(), p64, p32, floor=fl['p'])
            _check_state('k_cg_step_small', case, state, (0, 1, 2, 4), st64, st32, floors=fl)
        assert torch.equal(_bits(state.t[0:1]), _bits(state.before[4:5]))             # rho <- the rho this step used, a copy


# ---------------------------------------------------------------------------------------------------------------------------------
# 3c. short solves through GaussNewtonCG.run on a dense problem, every CG flag
# ---------------------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVE_FLAGS = list(itertools.product((False, True), (False, True), (0.0, 0.5)))         # fletcher_reeves, standard_alpha, dff


class _DenseProblem:
    """Stub problem of model/optimizer.py's protocol: q = A0 p + lam p with torch on the device, one independent right-hand side per
    Gauss-Newton iteration.  No persistent_args: the solver takes the chain of launches."""

    def __init__(self, A0, rhs, layout, small):
        self.A0, self.rhs, self.layout, self.k, self.after = _d(A0), [_d(b) for b in rhs], layout, 0, []
        self.slab = torch.empty(layout[0] + layout[1], device=DEV)
        if small:
            self.apply_A_partials = self._partials

    def initialize(self):
        pass

    def vector_layout(self):
        return self.layout

    def linearize(self, x, b):
        b.copy_(self.rhs[self.k])
        self.k += 1

    def apply_A(self, p, q):
        torch.mv(self.A0, p, out=self.slab)
        torch.add(self.slab, p, alpha=S.SOLVE_LAM, out=q)

    def _partials(self, p):
        torch.mv(self.A0, p, out=self.slab)
        return self.slab, 1, self.slab.numel(), S.SOLVE_LAM

    def apply_step(self, x, step, delta):
        o = 0
        for v in x:
            if v.numel():
                _call('frtm_vec_axpy', v, float(step), delta[o:o + v.numel()], v.numel())
            o += v.numel()
        self.after.append(torch.cat([v.reshape(-1) for v in x]).clone())

    def views(self, flat):
        from frtm_vos_amd.lib.tensorlist import TensorList
        n1 = self.layout[0]
        return TensorList([flat[:n1], flat[n1:]])


@pytest.fixture(scope='module')
def dense_refs():
    """Per layout: the inputs, and per flag set the float64 result after each Gauss-Newton iteration with the yardstick: the same
    GaussNewtonCGRef in fp32 on the CPU."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import cpu_ref as O
    out = {}
    for name, layout in S.SOLVE_LAYOUTS.items():
        A0, rhs = S.spd_problem(layout[0] + layout[1], 7 + len(name))
        per = {fl: tuple(S.dense_reference(O, A0, rhs, layout, *fl, dt) for dt in (torch.float64, torch.float32)) for fl in SOLVE_FLAGS}
        out[name] = (layout, A0, rhs, per)
    return out


@pytest.mark.parametrize('fr,sa,dff', SOLVE_FLAGS)
@pytest.mark.parametrize('name', ['small', 'multi'])
def test_short_solves(dense_refs, name, fr, sa, dff):
    """(864, 0) with apply_A_partials: frtm_cg_direction once, then frtm_cg_step_small; (1000, 37): the multi-kernel sequence.  Schedule
    (3, 4, 2); the accumulated variable after each Gauss-Newton iteration."""
    from frtm_vos_amd.lib.tensorlist import TensorList
    from frtm_vos_amd.model.optimizer import GaussNewtonCG
    layout, A0, rhs, per = dense_refs[name]
    ref64, ref32 = per[(fr, sa, dff)]
    pr = _DenseProblem(A0, rhs, layout, small=name == 'small')
    x = TensorList([torch.zeros(layout[0], device=DEV), torch.zeros(layout[1], device=DEV)])
    opt = GaussNewtonCG(pr, x, fletcher_reeves=fr, standard_alpha=sa, direction_forget_factor=dff)
    assert not opt._generic
    opt.run(S.SOLVE_SCHEDULE)
    torch.cuda.synchronize()
    assert len(pr.after) == len(S.SOLVE_SCHEDULE)
    for k, got in enumerate(pr.after):
        _check('solve %s' % name, 'fr %d sa %d dff %.1f gn %d' % (fr, sa, dff, k), got, ref64[k], ref32[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# 3d. the three joint forms and the filter form of DiscriminatorLoss against float64, off the fixture shapes
# ---------------------------------------------------------------------------------------------------------------------------------
JOINT_SHAPES = [(2, 20, 5, 5, 9), (3, 70, 18, 17, 31), (2, 36, 8, 6, 80)]            # N, Cin, c, h, w; the last: a map wider than a wavefront
REGS = (0.5, 0.7)                                                                    # lam = reg^2: large enough to show in b and A p


def _filled_memory(N, C, h, w):
    """A real Memory of N samples of (C, h, w) features with labels 16x the map and hinge pixel weights -> (memory, X, B, c, sw) with the
    operands read back from it (fp32, CPU): frtm_normal_build, which has tests of its own, is not re-judged here."""
    from frtm_vos_amd.model.memory import Memory
    g = _gen(N, C, h, w, 30)
    Hh, Ww = 16 * h, 16 * w
    x = torch.relu(_randn(g, N, C, h, w))
    Y = torch.zeros(N, 1, Hh, Ww, dtype=torch.uint8)
    for k in range(N):
        Y[k, 0, Hh // 5 + 4 * k:Hh // 5 + 4 * k + Hh // 4, Ww // 4:Ww // 2 + 6 * k] = 1
    mem = Memory(N, (C, h, w), (1, Hh, Ww), DEV, 0.1, pixel_weighting=dict(method='hinge', tf=0.1))
    mem.initialize(x.to(DEV), Y.to(DEV))
    torch.cuda.synchronize()
    X, B, c, sw = mem.samples[:N].cpu(), mem.normal_B[:N].cpu(), mem.normal_c[:N].cpu(), mem.weights[:N].cpu()
    assert torch.equal(X, x) and float(sw.min()) > 0 and float(sw.min()) < float(sw.max())
    return mem, X, B, c, sw


@pytest.mark.parametrize('form', ['chain', 'fused', 'composed'])
@pytest.mark.parametrize('N,Cin,c,h,w', JOINT_SHAPES)
def test_joint_forms_against_float64(form, N, Cin, c, h, w):
    """b after linearize, A p for one random p and (fused, composed: the forms that have it) apply_A_pq with r given -- q and both partial sums
    -- against the low-resolution joint operator of tests/_solver_refs.py."""
    from frtm_vos_amd.lib.tensorlist import TensorList
    from frtm_vos_amd.model.discriminator import DiscriminatorLoss
    from frtm_vos_amd.model.optimizer import GaussNewtonCG
    mem, X, B, cmap, sw = _filled_memory(N, Cin, h, w)
    g = _gen(N, Cin, c, h, w, 31)
    w1_0 = (torch.rand(c, Cin, 1, 1, generator=g) * 2 - 1) / Cin ** 0.5
    w2_0 = (torch.rand(1, c, 3, 3, generator=g) * 2 - 1) / (9 * c) ** 0.5
    n1, n2 = Cin * c, 9 * c
    pvec, r = _randn(g, n1 + n2) * 0.05, _randn(g, n1 + n2)
    w1 = torch.nn.Parameter(w1_0.clone().to(DEV), requires_grad=False)
    w2 = torch.nn.Parameter(w2_0.clone().to(DEV), requires_grad=False)
    prob = DiscriminatorLoss(mem, REGS, (1e-4, 1e-2), w2, w1)
    prob.composed, prob.fused, prob.persistent_joint = form == 'composed', form == 'fused', False
    opt = GaussNewtonCG(prob, TensorList([w1, w2]), fletcher_reeves=False, standard_alpha=True, direction_forget_factor=0.5)
    opt.persistent, opt.persistent_joint = False, False
    prob.initialize()
    assert prob._use_composed() == (form == 'composed') and prob._use_fused() == (form == 'fused') and prob.persistent_joint_args() is None
    opt._alloc()
    lam1, lam2 = REGS[0] ** 2, REGS[1] ** 2
    w1T, w2f = w1_0.reshape(c, Cin).t().contiguous(), w2_0.reshape(c, 9)
    case = '%s N%d Cin%d c%d %dx%d' % (form, N, Cin, c, h, w)

    b = _Buf(n1 + n2)
    prob.linearize(opt.x, b.t)
    b64, b32 = _legs(lambda *a: S.joint_rhs(*a, lam1, lam2), X, w1T, w2f, B, cmap, sw)
    _check('joint linearize', case, b.done(), b64, b32)

    def A(p_):
        return lambda X_, w1T_, w2_, B_, sw_, p__: S.joint_A(X_, w1T_, w2_, B_, sw_, lam1, lam2, p__[:n1].reshape(Cin, c), p__[n1:].reshape(c, 9))
    q64, q32 = _legs(A(pvec), X, w1T, w2f, B, sw, pvec)
    q = _Buf(n1 + n2)
    prob.apply_A(_d(pvec), q.t)
    _check('joint apply_A', case, q.done(), q64, q32)
    if form == 'chain':
        return
    q, partial = _Buf(n1 + n2), _Buf(4 * BLOCKS)
    prob.apply_A_pq(_d(pvec), q.t, _d(r), partial.t)
    _check_q_and_partials('joint apply_A_pq', case, q, partial, q64, q32, pvec, r)


@pytest.mark.parametrize('N,Cin,c,h,w', JOINT_SHAPES)
def test_filter_form_against_float64(N, Cin, c, h, w):
    """The filter-only problem on a memory of (c, h, w) features: b, A p, and the slabs of apply_A_partials reduced by frtm_vec_reduce_slabs."""
    from frtm_vos_amd.lib.tensorlist import TensorList
    from frtm_vos_amd.model.discriminator import DiscriminatorLoss
    from frtm_vos_amd.model.optimizer import GaussNewtonCG
    mem, X, B, cmap, sw = _filled_memory(N, c, h, w)
    g = _gen(N, c, h, w, 32)
    w2_0 = (torch.rand(1, c, 3, 3, generator=g) * 2 - 1) / (9 * c) ** 0.5
    pvec = _randn(g, 9 * c) * 0.05
    w2 = torch.nn.Parameter(w2_0.clone().to(DEV), requires_grad=False)
    prob = DiscriminatorLoss(mem, REGS[1:], (1e-2,), w2)
    opt = GaussNewtonCG(prob, TensorList([w2]), fletcher_reeves=False, standard_alpha=True, direction_forget_factor=0.5)
    opt.persistent = False
    prob.initialize()
    opt._alloc()
    lam = REGS[1] ** 2
    case = 'filter N%d c%d %dx%d' % (N, c, h, w)
    b = _Buf(9 * c)
    prob.linearize(opt.x, b.t)
    b64, b32 = _legs(lambda *a: S.filter_rhs(*a, lam), X, w2_0.reshape(c, 9), B, cmap, sw)
    _check('filter linearize', case, b.done(), b64, b32)
    q64, q32 = _legs(lambda X_, p_, B_, sw_: S.filter_A(X_, p_.reshape(c, 9), B_, sw_, lam), X, pvec, B, sw)
    q = _Buf(9 * c)
    prob.apply_A(_d(pvec), q.t)
    _check('filter apply_A', case, q.done(), q64, q32)
    slabs, nslab, stride, lam_ = prob.apply_A_partials(_d(pvec))
    assert abs(lam_ - lam) < 1e-12 and stride == 9 * c
    q = _Buf(9 * c)
    _call('frtm_vec_reduce_slabs', slabs, nslab, stride, 9 * c, float(lam_), _d(pvec), 1.0, q.t)
    _check('filter apply_A_partials', case, q.done(), q64, q32)
