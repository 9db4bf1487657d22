"""Every element-wise kernel of csrc/refiner_ops.hip and csrc/refiner_train.hip, forward and backward, against its float64 definition
(tests/_refiner_refs.py), called through the C entry points at the shapes the kernels branch on: tile and strip tails, channel-group
and unroll tails, the vector and scalar branches of the loads, z-slabs, grid-stride second trips, shared (`group`) planes.

Gate: the project's rule, tests/test_refiner_train_gpu.py::_gate,
    max|hip - ref64| <= max(4 * max|torch32 - ref64|, 1e-6 * max|ref64|)
with ref64 the reference in float64 on the CPU (on the GPU for the one large pyrup2x case) and torch32 the same expression in fp32 on
the GPU.  Inputs are fp32 values from a seeded CPU generator; both legs read exactly those values.

Three kernels evaluate the sigmoid with __expf (k_cab_combine, k_cab_bwd_shallow, k_cab_gate_bwd); for them the bound gains one term,
2^-21 * max|multiplicand| (the value that the sigmoid, or its derivative, multiplies), passed as the gate's floor.  Derivation:
__expf(-g) is exp2(-g * log2 e).  Rounding the scaled argument to fp32 moves it by at most half an ulp of a number below |g| * 1.4427,
which changes the exponential by a relative 0.37 * |g| * 2^-24 at most; the hardware exponential itself contributes about 1 ulp
(2^-24 relative).  A relative error r of e^-g changes the sigmoid by sigmoid' * r <= r / 4.  With |g| <= 4 (the gates drawn here) that is
(0.37 * 4 + 1) * 2^-24 / 4 < 2^-22 per unit of the multiplicand, and 2^-21 is a factor of two over it.

Output hygiene: every output buffer is pre-filled with NaN and sits between two guard bands of 64 floats, which must stay untouched;
an output that still holds a NaN was not written.

The ops.py wrappers of these entry points are held, bit for bit, to the direct call with hand-written dimensions (last section).

No test here asserts a time.  The module (314 tests before the wrapper cases) ran in 117 s on an MI355X in a fresh account (MIOpen choosing kernels for
the fp32 torch legs, the float64 legs on the CPU) and in 9 s with MIOpen's choices cached.
"""
import math

import pytest
import torch

import _refiner_refs as R
from test_refiner_train_gpu import _gate

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
NAN = float('nan')
EXPF_TERM = 2.0 ** -21


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _uniform(g, lo, hi, *shape):
    return torch.rand(*shape, generator=g) * (hi - lo) + lo


class _Out:
    """A NaN-filled output of `shape` between two guard bands; `skew` floats of extra offset (1: a view that is not 16-byte aligned)."""

    def __init__(self, *shape, skew=0):
        n = int(math.prod(shape))
        self.buf = torch.full((n + 2 * GUARD + skew,), NAN, device=DEV)
        self.lo = GUARD + skew
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == (4 * skew) % 16

    def done(self):
        """The guards are untouched and every element was written; returns the output."""
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:self.lo]).all()), 'write below the output'
        assert bool(torch.isnan(self.buf[self.lo + self.t.numel():]).all()), 'write above the output'
        assert not bool(torch.isnan(self.t).any()), 'output element not written'
        return self.t


def _skewed(x):
    """A copy of x on the GPU that starts one float past a 16-byte boundary."""
    buf = torch.empty(x.numel() + 1, device=DEV)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _check(kernel, case, hip, ref64, t32, floor=None):
    """The gate, with the figures printed first (`pytest -s` shows them): hip error, torch32 error, their ratio."""
    e = float((hip.double().cpu() - ref64.double().cpu()).abs().max())
    e32 = float((t32.double().cpu() - ref64.double().cpu()).abs().max())
    print('RATIO %s %s hip %.3e torch32 %.3e ratio %.3f max|ref| %.3e' % (kernel, case, e, e32, e / max(e32, 1e-30) if e else 0.0,
                                                                            float(ref64.abs().max())))
    assert hip.shape == ref64.shape
    _gate(hip, ref64, t32, '%s %s' % (kernel, case), floor=floor)


def _legs(fn, *args):
    """fn on the float64 copies of the (fp32, CPU) arguments on the CPU, and on their fp32 copies on the GPU."""
    def to(a, f):
        return f(a) if torch.is_tensor(a) else a
    r64 = fn(*[to(a, lambda t: t.double()) for a in args])
    r32 = fn(*[to(a, lambda t: t.to(DEV)) for a in args])
    return r64, r32


def _call(name, *args):
    from frtm_vos_amd import _hip as H
    H.call(name, *[H.ptr(a) if torch.is_tensor(a) else a for a in args])


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
RESIZES = [(13, 17, 13, 17), (13, 17, 40, 50), (15, 27, 30, 54), (20, 30, 9, 13), (1, 1, 7, 9), (1, 5, 3, 5), (30, 54, 60, 107),
           (60, 107, 120, 214)]


@pytest.mark.parametrize('planes', [1, 8, 9, 17])
@pytest.mark.parametrize('h,w,Ho,Wo', RESIZES)
def test_bilinear_resize(planes, h, w, Ho, Wo):
    x = _randn(_gen(planes, h, w, Ho), planes, h, w)
    out = _Out(planes, Ho, Wo)
    _call('frtm_bilinear_resize', x.to(DEV), planes, h, w, out.t, Ho, Wo)
    r64, r32 = _legs(lambda t: R.bilinear_resize(t, Ho, Wo), x)
    _check('k_bilinear_resize', '%dx(%d,%d)->(%d,%d)' % (planes, h, w, Ho, Wo), out.done(), r64, r32)


@pytest.mark.parametrize('h', [1, 2, 3, 4, 5, 7, 8, 9])
@pytest.mark.parametrize('w', [1, 2, 3, 64, 65])
def test_pyrup2x(h, w):
    planes = 3
    x = _randn(_gen(h, w), planes, h, w)
    out = _Out(planes, 2 * h, 2 * w)
    _call('frtm_pyrup2x', x.to(DEV), planes, h, w, out.t)
    r64, r32 = _legs(R.pyrup2x, x)
    _check('k_pyrup2x', '%dx%d' % (h, w), out.done(), r64, r32)


def test_pyrup2x_grid_stride_second_trip():
    """700 planes of 120 x 214: 700 * 30 * 214 column strips, more than the 16384 * 256 threads of the capped grid, so the last strips
    are the second trip of the grid-stride loop.  The float64 reference runs on the GPU (the CPU takes minutes at this size)."""
    planes, h, w = 700, 120, 214
    assert planes * ((h + 3) // 4) * w > 16384 * 256
    x = _randn(_gen(700), planes, h, w).to(DEV)
    out = _Out(planes, 2 * h, 2 * w)
    _call('frtm_pyrup2x', x, planes, h, w, out.t)
    hip = out.done()
    r64, r32 = R.pyrup2x(x.double()), R.pyrup2x(x)
    first = 16384 * 256 // (((h + 3) // 4) * w)                   # planes below this one belong to the first trip alone
    _check('k_pyrup2x', 'second trip, planes %d..' % (first + 1), hip[first + 1:], r64[first + 1:], r32[first + 1:])
    _check('k_pyrup2x', '700x120x214', hip, r64, r32)


MEAN_HW = [1, 3, 4, 221, 256, 1020, 1024, 1620, 25680]


@pytest.mark.parametrize('planes', [1, 70])
@pytest.mark.parametrize('HW,skew', [(hw, 0) for hw in MEAN_HW] + [(hw, 1) for hw in MEAN_HW if hw % 4 == 0])
def test_plane_mean(HW, skew, planes):
    """skew = 1: the same planes read through a view one float past a 16-byte boundary, the scalar branch for HW % 4 == 0 (with
    HW % 4 != 0 the scalar branch is taken either way)."""
    x = _randn(_gen(HW, planes), planes, HW) + 0.3
    xd = _skewed(x) if skew else x.to(DEV)
    out = _Out(planes)
    _call('frtm_plane_mean', xd, planes, HW, out.t)
    r64, r32 = _legs(R.plane_mean, x)
    _check('k_plane_mean', '%dx%d skew %d' % (planes, HW, skew), out.done(), r64, r32)


# (C, H, W, scores at half size, n, group); the last one is the production shape
TSE_CASES = [(1, 1, 1, False, 1, 1), (3, 8, 32, True, 3, 1), (4, 9, 33, False, 4, 2), (5, 7, 31, True, 6, 3), (64, 30, 54, True, 1, 1),
             (3, 61, 107, False, 4, 2), (5, 9, 33, True, 3, 1), (1, 61, 107, True, 6, 3), (4, 1, 1, True, 4, 2), (64, 8, 32, False, 3, 1),
             (5, 30, 54, False, 6, 3), (64, 60, 107, True, 4, 2)]


@pytest.mark.parametrize('C,Hh,Ww,half,n,group', TSE_CASES)
def test_tse_inject(C, Hh, Ww, half, n, group):
    g = _gen(C, Hh, Ww, n, group)
    h, w = ((Hh + 1) // 2, (Ww + 1) // 2) if half else (Hh, Ww)
    base = _randn(g, n // group, C, Hh, Ww)                       # one base map per frame, all different
    bias, ws, scores = _randn(g, C) * 0.5, _randn(g, C, 9) * 0.3, _randn(g, n, h, w)
    out = _Out(n, C, Hh, Ww)
    _call('frtm_tse_inject', base.to(DEV), bias.to(DEV), ws.to(DEV), scores.to(DEV), n, group, C, h, w, Hh, Ww, out.t)
    r64, r32 = _legs(lambda *a: R.tse_inject(*a, group), base, bias, ws, scores)
    _check('k_tse_inject', 'C%d %dx%d from %dx%d n%d g%d' % (C, Hh, Ww, h, w, n, group), out.done(), r64, r32)


@pytest.mark.parametrize('oc', [4, 8, 60, 64, 68, 256])
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('shared', [False, True])
def test_cab_gate(oc, n, shared):
    g = _gen(oc, n, shared)
    dp_group = n if shared else 0
    sp, dp = _randn(g, n, oc), _randn(g, 1 if shared else n, oc)
    W1, b1 = _randn(g, 2 * oc, oc) / (2 * oc) ** 0.5, _randn(g, oc) * 0.3
    W2, b2 = _randn(g, oc, oc) / oc ** 0.5, _randn(g, oc) * 0.3
    out = _Out(n, oc)
    _call('frtm_cab_gate', sp.to(DEV), dp.to(DEV), dp_group, W1.to(DEV), b1.to(DEV), W2.to(DEV), b2.to(DEV), n, oc, out.t)
    r64, r32 = _legs(lambda s, d, *a: R.cab_gate(s, d, dp_group, *a), sp, dp, W1, b1, W2, b2)
    _check('k_cab_gate', 'oc%d n%d group %d' % (oc, n, dp_group), out.done(), r64, r32)


# (n, C, hd, wd, deeper_group, H, W): same size; the pooled vector shared by the n samples; exact 2x; the pyramid's ratios; other ratios
COMBINE_CASES = [(2, 3, 1, 1, 0, 1, 1), (2, 3, 15, 63, 0, 15, 63), (2, 3, 16, 64, 0, 16, 64), (2, 3, 17, 65, 0, 17, 65), (2, 3, 33, 130, 0, 33, 130),
                 (3, 5, 1, 1, 3, 16, 64), (3, 5, 1, 1, 3, 17, 130), (3, 5, 1, 1, 3, 33, 1), (4, 2, 1, 1, 4, 1, 65), (6, 2, 1, 1, 3, 15, 63),
                 (2, 4, 8, 32, 0, 16, 64), (2, 4, 8, 65, 0, 16, 130), (1, 64, 15, 27, 0, 30, 54), (2, 8, 30, 54, 0, 60, 107),
                 (2, 2, 3, 7, 0, 15, 63), (2, 2, 5, 9, 0, 1, 65), (2, 2, 9, 1, 0, 33, 1), (2, 2, 40, 70, 0, 17, 65)]


@pytest.mark.parametrize('n,C,hd,wd,group,Hh,Ww', COMBINE_CASES)
def test_cab_combine(n, C, hd, wd, group, Hh, Ww):
    g = _gen(n, C, hd, wd, Hh, Ww)
    shallow, gate = _randn(g, n, C, Hh, Ww), _uniform(g, -4, 4, n, C)
    deeper = _randn(g, n // group if group else n, C, hd, wd)
    out = _Out(n, C, Hh, Ww)
    _call('frtm_cab_combine', shallow.to(DEV), gate.to(DEV), deeper.to(DEV), n, C, hd, wd, group, Hh, Ww, out.t)
    r64, r32 = _legs(lambda *a: R.cab_combine(*a, group), shallow, gate, deeper)
    _check('k_cab_combine', 'n%d C%d (%d,%d)->(%d,%d) g%d' % (n, C, hd, wd, Hh, Ww, group), out.done(), r64, r32,
           floor=EXPF_TERM * float(shallow.abs().max()))


@pytest.mark.parametrize('C', [1, 3, 4, 5, 32, 33])
@pytest.mark.parametrize('hw', [1, 255, 256, 1024, 1028, 25680])
@pytest.mark.parametrize('n', [1, 3])
def test_tap_mix(C, hw, n):
    g = _gen(C, hw, n)
    y, w = _randn(g, n, C, hw), _randn(g, C, 9) * 0.3
    out = _Out(n, 9, hw)
    _call('frtm_tap_mix', y.to(DEV), n, C, hw, w.to(DEV), out.t)
    r64, r32 = _legs(R.tap_mix, y, w)
    _check('k_tap_mix', 'C%d hw%d n%d' % (C, hw, n), out.done(), r64, r32)


@pytest.mark.parametrize('skew_in,skew_out', [(1, 0), (0, 1), (1, 1)])
def test_tap_mix_misaligned(skew_in, skew_out):
    """hw % 4 == 0 through views that are not 16-byte aligned: the scalar form must be taken for either pointer."""
    n, C, hw = 2, 5, 1024
    g = _gen(skew_in, skew_out, 9)
    y, w = _randn(g, n, C, hw), _randn(g, C, 9) * 0.3
    out = _Out(n, 9, hw, skew=skew_out)
    _call('frtm_tap_mix', _skewed(y) if skew_in else y.to(DEV), n, C, hw, w.to(DEV), out.t)
    r64, r32 = _legs(R.tap_mix, y, w)
    _check('k_tap_mix', 'skew in %d out %d' % (skew_in, skew_out), out.done(), r64, r32)


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 255, 257, 3 * 10 ** 6, 5 * 10 ** 6])
def test_relu_backward(n):
    """Exact.  y holds exact zeros and -0.0 (no gradient there); 5e6 elements pass the 16384 * 256 threads of the capped grid."""
    g = _gen(n)
    y, dy = _randn(g, n), _randn(g, n)
    y[::3] = 0.0
    y[1::7] = -0.0
    out = _Out(n)
    _call('frtm_relu_backward', dy.to(DEV), y.to(DEV), n, out.t)
    ref = R.relu_backward(dy.double(), y.double())
    assert int((ref == 0).sum()) >= n // 3
    print('RATIO k_relu_bwd n%d exact' % n)
    assert torch.equal(out.done().cpu(), ref.float())


@pytest.mark.parametrize('Hh,Ww', [(1, 1), (1, 5), (3, 1), (16, 16), (17, 33)])
@pytest.mark.parametrize('n', [1, 3])
def test_shift9(Hh, Ww, n):
    dl = _randn(_gen(Hh, Ww, n), n, Hh, Ww)
    out = _Out(n, 9, Hh, Ww)
    _call('frtm_shift9', dl.to(DEV), n, Hh, Ww, out.t)
    print('RATIO k_shift9 n%d %dx%d exact' % (n, Hh, Ww))
    assert torch.equal(out.done().cpu(), R.shift9(dl))


BWD_HW = [1, 255, 256, 257, 25680]


@pytest.mark.parametrize('planes', [1, 7])
@pytest.mark.parametrize('HW', [1, 255, 257, 25680])
def test_add_plane(planes, HW):
    g = _gen(planes, HW)
    x, v = _randn(g, planes, HW), _randn(g, planes) * HW ** 0.5
    out = _Out(planes, HW)                                        # in place: the output buffer starts as x
    out.t.copy_(x)
    _call('frtm_add_plane', out.t, v.to(DEV), 1.0 / HW, planes, HW)
    r64, r32 = _legs(lambda a, b: R.add_plane(a, b, 1.0 / HW), x, v)
    _check('k_add_plane', '%dx%d' % (planes, HW), out.done(), r64, r32)


@pytest.mark.parametrize('planes', [1, 130])
@pytest.mark.parametrize('HW', BWD_HW)
def test_cab_backward_reduce(planes, HW):
    g = _gen(planes, HW, 1)
    dout, s = _randn(g, planes, HW), _randn(g, planes, HW) + 0.5
    a, b = _Out(planes), _Out(planes)
    _call('frtm_cab_backward_reduce', dout.to(DEV), s.to(DEV), planes, HW, a.t, b.t)
    (a64, b64), (a32, b32) = _legs(R.cab_backward_reduce, dout, s)
    _check('k_cab_bwd_reduce', 'a %dx%d' % (planes, HW), a.done(), a64, a32)
    _check('k_cab_bwd_reduce', 'b %dx%d' % (planes, HW), b.done(), b64, b32)


@pytest.mark.parametrize('planes', [1, 130])
@pytest.mark.parametrize('HW', BWD_HW)
def test_cab_backward_shallow(planes, HW):
    g = _gen(planes, HW, 2)
    dout, gate, dsp = _randn(g, planes, HW), _uniform(g, -4, 4, planes), _randn(g, planes) * HW ** 0.5
    out = _Out(planes, HW)
    _call('frtm_cab_backward_shallow', dout.to(DEV), gate.to(DEV), dsp.to(DEV), planes, HW, out.t)
    r64, r32 = _legs(R.cab_backward_shallow, dout, gate, dsp)
    _check('k_cab_bwd_shallow', '%dx%d' % (planes, HW), out.done(), r64, r32, floor=EXPF_TERM * float(dout.abs().max()))


def _gate_bwd_inputs(oc, n):
    """Inputs of the gate backward.  b1 is moved, per hidden unit, until no float64 pre-activation lies within 1e-3 of zero, so that the
    fp32 evaluations cannot land on the other side of the ReLU: no kink is in play and no element needs excluding."""
    g = _gen(oc, n, 3)
    sp, dp = _randn(g, n, oc), _randn(g, n, oc)
    W1, b1 = _randn(g, oc, 2 * oc) / (2 * oc) ** 0.5, _randn(g, oc) * 0.3
    W2, b2 = _randn(g, oc, oc) / oc ** 0.5, _randn(g, oc) * 0.3
    for _ in range(200):
        near = (R.cab_gate_preact(sp.double(), dp.double(), W1.double(), b1.double()).abs() < 1e-3).any(0)
        if not bool(near.any()):
            break
        b1[near] += 0.0037
    pre = R.cab_gate_preact(sp.double(), dp.double(), W1.double(), b1.double())
    assert float(pre.abs().min()) >= 1e-4, 'a pre-activation within 1e-4 of the ReLU kink'
    assert bool((pre > 0).any()) and (oc * n < 16 or bool((pre < 0).any()))         # both sides of the ReLU occur
    gate = torch.relu(pre) @ W2.double().t() + b2.double()
    shrink = min(1.0, 3.9 / float(gate.abs().max()))               # |gate| <= 4 by construction (the derived term assumes it): the gate is
    W2, b2 = W2 * shrink, b2 * shrink                               # linear in W2 and b2, so scaling both scales it
    gate = (torch.relu(pre) @ W2.double().t() + b2.double()).float()               # the forward's gate, as the backward receives it
    assert float(gate.abs().max()) <= 4.0
    a, badd = _randn(g, n, oc), _randn(g, n, oc)
    return sp, dp, gate, a, badd, W1, b1, W2


def _run_gate_bwd(oc, n, sp, dp, gate, a, badd, W1, b1, W2, weight_grads=True):
    outs = [_Out(oc, 2 * oc), _Out(oc), _Out(oc, oc), _Out(oc)] if weight_grads else [None] * 4
    dsp, ddp = _Out(n, oc), _Out(n, oc)
    _call('frtm_cab_gate_backward', sp.to(DEV), dp.to(DEV), gate.to(DEV), a.to(DEV), None if badd is None else badd.to(DEV), W1.to(DEV),
          b1.to(DEV), W2.to(DEV), n, oc, *[o.t if o is not None else None for o in outs], dsp.t, ddp.t)
    return [o.done() if o is not None else None for o in outs + [dsp, ddp]]


@pytest.mark.parametrize('oc', [4, 8, 64])
@pytest.mark.parametrize('n', [1, 2, 5, 16])
@pytest.mark.parametrize('with_badd', [False, True])
def test_cab_gate_backward(oc, n, with_badd):
    sp, dp, gate, a, badd, W1, b1, W2 = _gate_bwd_inputs(oc, n)
    badd = badd if with_badd else None
    got = _run_gate_bwd(oc, n, sp, dp, gate, a, badd, W1, b1, W2)
    r64, r32 = _legs(R.cab_gate_backward, sp, dp, gate, a, badd, W1, b1, W2)
    for name, h, x64, x32 in zip(('dW1', 'db1', 'dW2', 'db2', 'dsp', 'ddp'), got, r64, r32):
        _check('k_cab_gate_bwd', '%s oc%d n%d badd %d' % (name, oc, n, with_badd), h, x64, x32, floor=EXPF_TERM * float(a.abs().max()))


def test_cab_gate_backward_frozen_weights():
    """All four weight-gradient pointers NULL (frozen parameters): dsp and ddp are bit for bit those of the full call."""
    oc, n = 64, 5
    args = _gate_bwd_inputs(oc, n)
    full = _run_gate_bwd(oc, n, *args)
    frozen = _run_gate_bwd(oc, n, *args, weight_grads=False)
    assert frozen[:4] == [None] * 4
    assert torch.equal(frozen[4], full[4]) and torch.equal(frozen[5], full[5])
    r64, r32 = _legs(R.cab_gate_backward, *args)
    for name, h, x64, x32 in zip(('dsp', 'ddp'), frozen[4:], r64[4:], r32[4:]):
        _check('k_cab_gate_bwd', '%s frozen' % name, h, x64, x32, floor=EXPF_TERM * float(args[3].abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: each from the argument check itself (its message), with buffers that are valid for the call
# ---------------------------------------------------------------------------------------------------------------------------------
def _z(*shape):
    return torch.zeros(*shape, device=DEV)


@pytest.mark.parametrize('h,w,Hh,Ww', [(0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-1, 1, 1, 1)])
def test_tse_inject_refuses_empty_maps(h, w, Hh, Ww):
    with pytest.raises(RuntimeError, match='frtm_tse_inject: map sizes must be positive'):
        _call('frtm_tse_inject', _z(1, 1, 1, 1), _z(1), _z(1, 9), _z(1, 1, 1), 1, 1, 1, h, w, Hh, Ww, _z(1, 1, 1, 1))


def test_tse_inject_refuses_maps_beyond_the_grid_and_the_index_range():
    """Both checks return before any launch, so one-element buffers serve."""
    one = lambda: _z(1, 1, 1, 1)
    with pytest.raises(RuntimeError, match='frtm_tse_inject: at most 524280 rows'):
        _call('frtm_tse_inject', one(), _z(1), _z(1, 9), _z(1, 1, 1), 1, 1, 1, 1, 1, 65535 * 8 + 1, 1, one())
    with pytest.raises(RuntimeError, match='frtm_tse_inject: map too large'):
        _call('frtm_tse_inject', one(), _z(1), _z(1, 9), _z(1, 1, 1), 1, 1, 1, 1, 1, 50000, 50000, one())
    with pytest.raises(RuntimeError, match='frtm_tse_inject: map too large'):
        _call('frtm_tse_inject', one(), _z(1), _z(1, 9), _z(1, 1, 1), 1, 1, 1, 50000, 50000, 1, 1, one())


def test_bilinear_resize_refuses_maps_beyond_the_index_range():
    for h, w, Ho, Wo in ((50000, 50000, 1, 1), (1, 1, 50000, 50000)):
        with pytest.raises(RuntimeError, match='frtm_bilinear_resize: map too large'):
            _call('frtm_bilinear_resize', _z(1, 1, 1), 1, h, w, _z(1, 1, 1), Ho, Wo)


def test_cab_gate_refuses_bad_groups():
    args = lambda n: (_z(n, 4), _z(n, 4))
    tail = (_z(8, 4), _z(4), _z(4, 4), _z(4))
    with pytest.raises(RuntimeError, match='frtm_cab_gate: dp_group must not be negative'):
        _call('frtm_cab_gate', *args(2), -1, *tail, 2, 4, _z(2, 4))
    with pytest.raises(RuntimeError, match='frtm_cab_gate: 3 samples are not a multiple of dp_group 2'):
        _call('frtm_cab_gate', *args(3), 2, *tail, 3, 4, _z(3, 4))


def test_tse_inject_refuses_more_samples_than_the_grid_holds():
    n = 16384                                                    # n * 4 channel groups = 65536 > 65535
    with pytest.raises(RuntimeError, match='frtm_tse_inject: at most 16383 samples'):
        _call('frtm_tse_inject', _z(n, 1, 1, 1), _z(1), _z(1, 9), _z(n, 1, 1), n, 1, 1, 1, 1, 1, 1, _z(n, 1, 1, 1))
    out = _Out(n - 1, 1, 1, 1)                                    # the largest count that fits still runs
    _call('frtm_tse_inject', _z(n - 1, 1, 1, 1), torch.ones(1, device=DEV), _z(1, 9), _z(n - 1, 1, 1), n - 1, 1, 1, 1, 1, 1, 1, out.t)
    assert bool((out.done() == 1).all())


def test_project_tail_refuses_more_samples_than_the_grid_holds():
    n = 65536
    with pytest.raises(RuntimeError, match='frtm_project_tail: at most 65535 samples'):
        _call('frtm_project_tail', _z(n, 1, 2, 2), n, 1, 2, 2, _z(1, 9), _z(1), 4, 4, _z(n, 1, 4, 4))


def test_tap_mix_refuses_more_samples_than_the_grid_holds():
    n = 65536
    with pytest.raises(RuntimeError, match='frtm_tap_mix: at most 65535 samples'):
        _call('frtm_tap_mix', _z(n, 1, 1), n, 1, 1, _z(1, 9), _z(n, 9, 1))


def test_bilinear_resize_refuses_more_planes_than_the_grid_holds():
    planes = 65535 * 8 + 1
    with pytest.raises(RuntimeError, match='frtm_bilinear_resize: at most 524280 planes'):
        _call('frtm_bilinear_resize', _z(planes, 1, 1), planes, 1, 1, _z(planes, 1, 1), 1, 1)


def test_cab_gate_refuses_oc_beyond_a_default_launch():
    """7 * oc floats of dynamic LDS: 2340 channels are the most that 65536 bytes hold; the largest width that fits still runs."""
    oc = 2344
    with pytest.raises(RuntimeError, match='frtm_cab_gate: oc = 2344 needs 65632 bytes of LDS'):
        _call('frtm_cab_gate', _z(1, oc), _z(1, oc), 0, _z(2 * oc, oc), _z(oc), _z(oc, oc), _z(oc), 1, oc, _z(1, oc))
    with pytest.raises(RuntimeError, match='multiple of 4'):
        _call('frtm_cab_gate', _z(1, 6), _z(1, 6), 0, _z(12, 6), _z(6), _z(6, 6), _z(6), 1, 6, _z(1, 6))
    oc, n = 2340, 2
    g = _gen(oc)
    sp, dp = _randn(g, n, oc), _randn(g, n, oc)
    W1, b1 = _randn(g, 2 * oc, oc) / (2 * oc) ** 0.5, _randn(g, oc) * 0.3
    W2, b2 = _randn(g, oc, oc) / oc ** 0.5, _randn(g, oc) * 0.3
    out = _Out(n, oc)
    _call('frtm_cab_gate', sp.to(DEV), dp.to(DEV), 0, W1.to(DEV), b1.to(DEV), W2.to(DEV), b2.to(DEV), n, oc, out.t)
    r64, r32 = _legs(lambda s, d, *a: R.cab_gate(s, d, 0, *a), sp, dp, W1, b1, W2, b2)
    _check('k_cab_gate', 'oc%d n%d (largest)' % (oc, n), out.done(), r64, r32)


def test_cab_combine_refuses_empty_maps_and_ragged_groups():
    with pytest.raises(RuntimeError, match='frtm_cab_combine: map sizes must be positive'):
        _call('frtm_cab_combine', _z(1, 1, 1, 1), _z(1, 1), _z(1, 1, 1, 1), 1, 1, 0, 1, 0, 1, 1, _z(1, 1, 1, 1))
    with pytest.raises(RuntimeError, match='frtm_cab_combine: 3 samples are not a multiple of deeper_group 2'):
        _call('frtm_cab_combine', _z(3, 1, 1, 1), _z(3, 1), _z(2, 1, 1, 1), 3, 1, 1, 1, 2, 1, 1, _z(3, 1, 1, 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# the ops.py wrappers: each derives the integers of its launch from the tensor shapes; here every one is held, bit for bit, to the direct
# call with the dimensions written out by hand.  No two dimensions coincide (n = 6 in groups of 3, C = 8, maps 5 x 7 -> 9 x 13, image
# 18 x 26), so a transposed pair shows.
# ---------------------------------------------------------------------------------------------------------------------------------
def _wrapper_case(name):
    from frtm_vos_amd import ops
    g = _gen(*name.encode())
    d = lambda *shape: _randn(g, *shape).to(DEV)
    n, grp, C, h, w, Hh, Ww, Ho, Wo = 6, 3, 8, 5, 7, 9, 13, 18, 26
    if name == 'plane_mean':
        x, o = d(n, C, Hh, Ww), _Out(n, C)
        _call('frtm_plane_mean', x, 48, 117, o.t)
        return ops.plane_mean(x), o
    if name == 'pyrup2x':
        x, o = d(n, C, h, w), _Out(n, C, 10, 14)
        _call('frtm_pyrup2x', x, 48, 5, 7, o.t)
        return ops.pyrup2x(x), o
    if name == 'bicubic_resize':
        x, o = d(n, C, h, w), _Out(n, C, Hh, Ww)
        _call('frtm_bicubic_resize', x, 48, 5, 7, o.t, 9, 13)
        return ops.bicubic_resize(x, (Hh, Ww)), o
    if name == 'tse_inject':
        base, bias, ws, scores, o = d(2, C, Hh, Ww), d(C), d(C, 9), d(n, 1, h, w), _Out(n, C, Hh, Ww)
        _call('frtm_tse_inject', base, bias, ws, scores, 6, 3, 8, 5, 7, 9, 13, o.t)
        return ops.tse_inject(base, bias, ws, scores, grp), o
    if name in ('cab_gate', 'cab_gate_shared'):
        shared = name == 'cab_gate_shared'
        sp, dp, W1, b1, W2, b2, o = d(n, C), d(2 if shared else n, C), d(2 * C, C), d(C), d(C, C), d(C), _Out(n, C)
        _call('frtm_cab_gate', sp, dp, 3 if shared else 0, W1, b1, W2, b2, 6, 8, o.t)
        return ops.cab_gate(sp, dp, W1, b1, W2, b2, dp_group=grp if shared else 0), o
    if name == 'cab_combine':
        shallow, gate, deeper, o = d(n, C, Hh, Ww), d(n, C), d(n, C, h, w), _Out(n, C, Hh, Ww)
        _call('frtm_cab_combine', shallow, gate, deeper, 6, 8, 5, 7, 0, 9, 13, o.t)
        return ops.cab_combine(shallow, gate, deeper), o
    if name == 'cab_combine_pooled':
        shallow, gate, pooled, o = d(n, C, Hh, Ww), d(n, C), d(2, C), _Out(n, C, Hh, Ww)
        _call('frtm_cab_combine', shallow, gate, pooled, 6, 8, 1, 1, 3, 9, 13, o.t)
        return ops.cab_combine(shallow, gate, pooled, deeper_group=grp), o
    if name == 'tap_mix':
        y, w2, o = d(n, C, Hh, Ww), d(1, C, 3, 3), _Out(n, 9, Hh, Ww)
        _call('frtm_tap_mix', y, 6, 8, 117, w2, o.t)
        return ops.tap_mix(y, w2), o
    if name in ('project_tail', 'project_tail_bicubic', 'project_tail_no_bias'):
        y, w2, o = d(n, C, Hh, Ww), d(1, C, 3, 3), _Out(n, 1, Ho, Wo)
        bias = None if name == 'project_tail_no_bias' else d(1)
        assert ops.project_tail_fits(Hh, Ww, (Ho, Wo), name == 'project_tail_bicubic')
        _call('frtm_' + name.replace('_no_bias', ''), y, 6, 8, 9, 13, w2, bias, 18, 26, o.t)
        return ops.project_tail(y, w2, bias, (Ho, Wo), bicubic=name == 'project_tail_bicubic'), o
    if name == 'shift9':
        dl, o = d(n, 1, Ho, Wo), _Out(n, 9, Ho, Wo)
        _call('frtm_shift9', dl, 6, 18, 26, o.t)
        return ops.shift9(dl), o
    if name == 'cab_backward_reduce':
        dout, s, a, b = d(n, C, Hh, Ww), d(n, C, Hh, Ww), _Out(n, C), _Out(n, C)
        _call('frtm_cab_backward_reduce', dout, s, 48, 117, a.t, b.t)
        return ops.cab_backward_reduce(dout, s), (a, b)
    if name in ('cab_gate_backward', 'cab_gate_backward_frozen'):
        frozen = name.endswith('frozen')
        sp, dp, gate, a, W1, b1, W2 = d(n, C), d(n, C), d(n, C), d(n, C), d(C, 2 * C, 1, 1), d(C), d(C, C, 1, 1)
        badd = None if frozen else d(n, C)
        outs = [None] * 4 if frozen else [_Out(C, 2 * C, 1, 1), _Out(C), _Out(C, C, 1, 1), _Out(C)]
        outs += [_Out(n, C), _Out(n, C)]
        _call('frtm_cab_gate_backward', sp, dp, gate, a, badd, W1, b1, W2, 6, 8, *[o if o is None else o.t for o in outs])
        return ops.cab_gate_backward(sp, dp, gate, a, badd, W1, b1, W2, grads=(not frozen,) * 4), outs
    if name == 'cab_backward_shallow':
        dout, gate, dsp, o = d(n, C, Hh, Ww), d(n, C), d(n, C), _Out(n, C, Hh, Ww)
        _call('frtm_cab_backward_shallow', dout, gate, dsp, 48, 117, o.t)
        return ops.cab_backward_shallow(dout, gate, dsp), o
    raise KeyError(name)


@pytest.mark.parametrize('name', ['plane_mean', 'pyrup2x', 'bicubic_resize', 'tse_inject', 'cab_gate', 'cab_gate_shared', 'cab_combine', 'cab_combine_pooled',
                                  'tap_mix', 'project_tail', 'project_tail_bicubic', 'project_tail_no_bias', 'shift9', 'cab_backward_reduce',
                                  'cab_gate_backward', 'cab_gate_backward_frozen', 'cab_backward_shallow'])
def test_wrapper_equals_the_direct_call(name):
    got, want = _wrapper_case(name)
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want)
    for a, o in zip(got, want):
        if o is None:
            assert a is None
            continue
        b = o.done()
        assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous()
        assert torch.equal(a, b), name
