"""The kernels of the refiner's training step that sum -- csrc/refiner_train.hip: the fp32 MFMA weight gradient and its slab reduce, the five
BatchNorm kernels; the input gradient that model/refiner_train.py builds from flipped weights; csrc/train_step.hip: the edges of the loss tail,
of the scale and of the Adam kernel -- against their float64 definitions (tests/_train_refs.py, pinned by tests/test_train_refs.py, which also
shows that these inputs tell seven wrong kernels from the right one), called through the C entry points with hand-written dimensions.

The apparatus is that of tests/test_solver_kernels_gpu.py and tests/test_target_data_gpu.py: the gate tests/test_refiner_train_gpu.py::_gate,
    max|hip - ref64| <= max(4 * max|torch32 - ref64|, 1e-6 * max|ref64|),
the three legs reading the same fp32 values of a seeded CPU generator (eps and the BatchNorm factor as the fp32 values the kernels hold); every
output and workspace NaN-filled between two guard bands of 64 floats (_Buf: done() = every word written, same() = no word changed, bit for
bit); integer outputs between guard bands of a sentinel (_IntBuf) and compared exactly; `RATIO` printed for each check (`pytest -s`).

Which branch each shape reaches:
  frtm_conv_wgrad (Cout, Cin, k, B, H, W)
    (1,1,1,1,1,1), (1,1,3,1,1,1)     K = B H W = 1: one stage with 31 idle pixels; under 3 x 3 only the centre tap is inside the map
    (3,2,3,1,1,33)                   H = 1; K = 33: the second stage holds one pixel
    (5,7,3,2,5,1)                    W = 1; ncol = 64: the bias column is the last column of a tile; a stage spans both samples
    (63,63,1,1,8,16), (64,7,3,1,8,16)   K = 128 exactly: the chain is flushed at the end and acc is zero when the result is written; ncol = 64
    (65,64,1,2,9,15)                 ncol = 65: the bias column alone in a new tile; Cout = 65; three splits of 96, the last holding 78
    (129,65,3,3,7,11)                three row tiles, ten column tiles, two splits, a ragged last split, sample boundaries inside stages
    (64,64,3,1,16,16)                ncol - 1 = 576 = 9 x 64; two full chains
    (1,1,1,2,37,45)                  27 splits, the last holding two pixels; also the aliased call dy is x with dw = NULL of refiner_train.py
    (9,32,1,2,24,43)                 17 splits, a last split of 16 pixels
    (4096,228,3,1,16,16)             2112 tiles: the 2048-tile budget gives zero splits and the clamp sets one
  Every shape: both outputs, dw alone, dbias alone (the other pointer NULL, its memory untouched), two calls bit for bit, a workspace of exactly
  frtm_conv_wgrad_ws_elems floats (every word of it written, the bands untouched), one float fewer refused with every output still NaN.
  k_conv_wgrad_reduce indexes with the int product Cout x ncol; the refiner's largest weight gradient (64 x 18433) is far from 2^31, and that
  limit is not tested here.
  frtm_bn_stats / frtm_bn_apply_relu / frtm_bn_relu_backward (N, C, HW)
    (1,1,1), (1,256,1)               cnt = 1: the `else var` branch of the unbiased variance; 256 channels: one full block of k_bn_stats_final
    (3,1,1), (3,257,1)               HW = 1 with cnt = 3; N C = 771 planes of one pixel; C = 257: the second block of k_bn_stats_final
    (1,1,255), (3,256,255)           HW < 256: idle threads in every plane sum; N = 1
    (3,64,257), (1,257,257)          HW = 257: a second trip of one thread, a second apply block of one pixel
    (1,64,25680)                     the refiner's 120 x 214 map
  Where C > 3, channel 1 is an offset plane (100 + 0.01 randn), channel 2 a constant plane (variance 0, invstd = 1 / sqrt(eps)), channel 3 has a
  beta that kills every pixel (dx, dgamma, dbeta of it exactly 0); elsewhere about half the pixels are dead.  Modes: train with factor 0.1, with
  the 1 / n factor of a first step (1), with 0 (running buffers bit for bit), with both running buffers NULL; eval with and without `part`;
  the backward also with dgamma = dbeta = NULL.  Each launch is checked on its own: apply and backward read the fp32 mean and invstd that the
  stats launch wrote, and the backward the fp32 `out` of the apply launch, in all three legs.
  _Runner.dgrad: (cin, cout, k) = (65,65,3) whole and with rows = 64, (64,32,3), (64,64,1), (32,1,3) on maps 1 x 1, 1 x 7, 5 x 1 (B = 2) and
  37 x 53 with the smallest B at which ops.wino_launch admits the 3 x 3 launch, with and without residual, net.use_winograd on and off.
  frtm_bce_logits (N, HW): (5, 1 / 2 / 3 / 5 / 7): no vector body, the scalar heads of the samples rotate through 0, 3, 2, 1; (130, 7): the
  waves of k_bce_final loop and the sample sum takes a second trip; (1, 260 x 256): P = 65, one lane takes a second partial.  uint8 and float
  targets, both definitions, dlogits = NULL.
  frtm_scale_by: n = 0, 1, 3, 4, 5, 1027, 2048 x 256 x 4 + 7 (tail only, body only, the second grid-stride trip with a tail).
  frtm_adam_amsgrad: lengths 1, 3, 2047, 2048, 2049, 4100 with vec = 1 and, one float past a 16-byte boundary, with vec = 0; 2049 x 2048 + 5
  elements: 2050 chunks, the grid-stride trip; the table entries (-1, 0), (ntens, 0) and (0, a chunk beyond n) that the three guards skip; a
  tensor that no entry names.

No floor above the plain gate was needed and no fault was found.  One thing in csrc changed with this module: k_bn_bwd_part / k_bn_bwd_apply
(csrc/refiner_train.hip) gained a third partial, sum xhat, and dx takes the mean of xhat out of its last term.  test_batchnorm_backward_sum_dx
shows it: before, at (3,64,257), (1,257,257) and (3,257,1), |sum dx| was 1.047, 1.062 and 1.946 of its bound (largest: the offset plane,
|sum dx| = 2.6 on the 120 x 214 map), because xhat is centred on the fp32 mean, which lies up to half an ulp = 2^-24 |mean| from the mean of x, and
sum dx = -gamma invstd^2 (sum g xhat) (mean64 - mean32) to first order.  After, the share of the bound per size is
    (1,1,1) 0   (3,1,1) 0.386   (1,1,255) 0.026   (3,64,257) 0.072   (1,64,25680) 0.011   (3,256,255) 0.103   (1,257,257) 0.117   (3,257,1) 0.633
    (1,256,1) 0
and at most 0.78 of the rounding term alone.  The definition (tests/_train_refs.py) takes the same mean out; in float64 it still equals
nn.BatchNorm2d's gradient.

No test here asserts a time.  The module (158 tests) ran in 7.8 s on an MI355X; the slowest test, one Adam table with its 4.2 million element
tensor, took 0.9 s.  Largest RATIO (hip error / torch32 error) per kernel; ratios above 4 passed on the 1e-6 floor of max|ref|:
    k_conv_wgrad dW 1.00, dbias 4.24 (65,64,1,2,9,15: 1.0e-5 on sums up to 50, a chain of 96 fp32 additions against torch's tree sum)
    k_bn_stats_final mean, invstd, running_mean, running_var 1.00   k_bn_apply_relu 2.61   k_bn_bwd_apply dx, dgamma, dbeta 1.00 (the fp64 sums:
    never behind the fp32 leg)   dgrad 2.44 on the direct route, 1.89 on the Winograd route
    k_bce_logits loss 1.00, dz 1.09   k_adam p 1.19, m 15.5 and v 15.0 (3.3e-7 of max|m|: b1 m + (1 - b1) g against torch's lerp), vmax 1.66
    frtm_scale_by, the counts, the guard bands and every word a launch must not write: exact.
"""
import pytest
import torch

import _train_refs as T
from test_solver_kernels_gpu import DEV, GUARD, NAN, _Buf, _bits, _call, _check, _d, _legs
from test_target_data_gpu import _IntBuf, _f32
from test_train_step_gpu import _logits, _targets

pytestmark = pytest.mark.gpu


def _lib():
    from frtm_vos_amd import _hip as H
    return H.lib()


def _ids(s):
    return 'x'.join(map(str, s))


# ---------------------------------------------------------------------------------------------------------------------------------
# 3a. weight gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def _wgrad(xd, dyd, shape, dw, db, ws, ws_elems=None):
    Cout, Cin, k, B, H, W = shape
    _call('frtm_conv_wgrad', dyd, xd, B, Cout, Cin, k, H, W, dw.t if dw else None, db.t if db else None, ws.t,
          ws.t.numel() if ws_elems is None else ws_elems)


@pytest.mark.parametrize('shape', T.WGRAD_SHAPES, ids=_ids)
def test_conv_wgrad(shape):
    Cout, Cin, k, B, H, W = shape
    ncol = Cin * k * k + 1
    x, dy = T.wgrad_inputs(*shape)
    (w64, b64), (w32, b32) = _legs(lambda x_, dy_: T.conv_wgrad(x_, dy_, k), x, dy)
    elems = _lib().frtm_conv_wgrad_ws_elems(B, Cout, Cin, k, H, W)
    nsplit = T.wgrad_plan(Cout, ncol, B * H * W)[0]
    assert elems == nsplit * Cout * ncol
    xd, dyd = _d(x), _d(dy)

    def bufs():
        return _Buf(Cout, Cin, k, k), _Buf(Cout), _Buf(elems)
    dw, db, ws = bufs()
    _wgrad(xd, dyd, shape, dw, db, ws)
    ws.done()                                                     # every slab word of every split, between untouched bands
    case = _ids(shape) + ' splits %d' % nsplit
    _check('k_conv_wgrad', 'dW ' + case, dw.done(), w64, w32)
    _check('k_conv_wgrad', 'dbias ' + case, db.done(), b64, b32)
    dw2, db2, ws2 = bufs()
    _wgrad(xd, dyd, shape, dw2, db2, ws2)
    assert torch.equal(_bits(dw2.done()), _bits(dw.t)) and torch.equal(_bits(db2.done()), _bits(db.t)) and torch.equal(_bits(ws2.done()), _bits(ws.t))
    dw3, db3, ws3 = bufs()
    _wgrad(xd, dyd, shape, dw3, None, ws3)
    assert torch.equal(_bits(dw3.done()), _bits(dw.t))
    db3.same()
    dw4, db4, ws4 = bufs()
    _wgrad(xd, dyd, shape, None, db4, ws4)
    assert torch.equal(_bits(db4.done()), _bits(db.t))
    dw4.same()
    dw5, db5, ws5 = bufs()
    with pytest.raises(RuntimeError, match='frtm_conv_wgrad: workspace of %d floats, need %d' % (elems - 1, elems)):
        _wgrad(xd, dyd, shape, dw5, db5, ws5, ws_elems=elems - 1)
    dw5.same(), db5.same(), ws5.same()


def test_conv_wgrad_aliased_bias_only():
    """refiner_train.py: conv_wgrad(dl, dl, 1, weight=False) -- dy and x are one tensor, Cin = Cout = 1, dw = NULL: the sum of dl."""
    shape = (1, 1, 1, 2, 37, 45)
    dl = T.wgrad_inputs(*shape)[1]
    r64, r32 = _legs(lambda t: t.sum().reshape(1), dl)
    dld = _Buf(init=dl)
    db, ws = _Buf(1), _Buf(_lib().frtm_conv_wgrad_ws_elems(2, 1, 1, 1, 37, 45))
    _wgrad(dld.t, dld.t, shape, None, db, ws)
    dld.same()
    _check('k_conv_wgrad', 'aliased dy is x, dbias only', db.done(), r64, r32)
    ws.done()


def test_conv_wgrad_refusals():
    x, dy = _d(torch.zeros(1, 2, 3, 4)), _d(torch.zeros(1, 3, 3, 4))
    dw, db, ws = _Buf(3, 2, 3, 3), _Buf(3), _Buf(1024)
    with pytest.raises(RuntimeError, match='frtm_conv_wgrad: kernel size must be 1 or 3'):
        _call('frtm_conv_wgrad', dy, x, 1, 3, 2, 2, 3, 4, dw.t, db.t, ws.t, 1024)
    with pytest.raises(RuntimeError, match='frtm_conv_wgrad: bad argument'):
        _call('frtm_conv_wgrad', dy, x, 1, 3, 2, 3, 3, 4, None, None, ws.t, 1024)
    for dims in ((0, 3, 2, 3, 3, 4), (1, 0, 2, 3, 3, 4), (1, 3, 0, 3, 3, 4), (1, 3, 2, 3, 0, 4), (1, 3, 2, 3, 3, 0)):
        with pytest.raises(RuntimeError, match='frtm_conv_wgrad: bad argument'):
            _call('frtm_conv_wgrad', dy, x, *dims, dw.t, db.t, ws.t, 1024)
        assert _lib().frtm_conv_wgrad_ws_elems(*dims) == 0
    assert _lib().frtm_conv_wgrad_ws_elems(1, 3, 2, 2, 3, 4) == 0
    dw.same(), db.same(), ws.same()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3b. BatchNorm + ReLU
# ---------------------------------------------------------------------------------------------------------------------------------
EPS = _f32(T.BN_EPS)
# (name, train, factor, running buffers, part)
BN_MODES = [('train f 0.1', 1, _f32(0.1), True, True), ('train f 1/n', 1, 1.0, True, True), ('train f 0', 1, 0.0, True, True),
            ('train no running', 1, _f32(0.1), False, True), ('eval', 0, 0.0, True, True), ('eval part NULL', 0, 0.0, True, False)]


class _part:
    """_Buf for the fp64 partials of a BatchNorm launch (2 N C for the statistics, 3 N C for the backward): NaN-filled doubles between two
    guard bands."""

    def __init__(self, N, C, per=2):
        n = per * N * C
        self.buf = torch.full((n + 2 * GUARD,), NAN, dtype=torch.float64, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]

    def guards(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.t.numel():]).all()), 'write beside the partials'

    def done(self):
        self.guards()
        assert not bool(torch.isnan(self.t).any()), 'partial not written'

    def same(self):
        self.guards()
        assert bool(torch.isnan(self.t).all()), 'a partial that the launch must not write has changed'


def _bn_forward(d, N, C, HW, train, factor, running, with_part, case):
    """frtm_bn_stats and frtm_bn_apply_relu, each against the definition; returns (mean, invstd, out) as the fp32 CPU tensors the launches wrote."""
    xd = _d(d['x'])
    rm, rv = (_Buf(init=d['rmean']), _Buf(init=d['rvar'])) if running else (None, None)
    mean, invstd, part = _Buf(C), _Buf(C), (_part(N, C) if with_part else None)
    _call('frtm_bn_stats', xd, N, C, HW, EPS, factor, train, rm.t if rm else None, rv.t if rv else None, mean.t, invstd.t, part.t if part else None)
    r64, r32 = _legs(lambda x_, rm_, rv_: T.bn_stats(x_, rm_, rv_, EPS, factor, train), d['x'], d['rmean'] if running else None,
                     d['rvar'] if running else None)
    _check('k_bn_stats_final', 'mean ' + case, mean.done(), r64[0], r32[0])
    _check('k_bn_stats_final', 'invstd ' + case, invstd.done(), r64[1], r32[1])
    if part is not None:
        part.done() if train else part.same()
    if running and train and factor != 0:
        _check('k_bn_stats_final', 'running_mean ' + case, rm.done(), r64[2], r32[2])
        _check('k_bn_stats_final', 'running_var ' + case, rv.done(), r64[3], r32[3])
    elif running:
        rm.same(), rv.same()
    if train and C > 3:
        assert float(invstd.t[T.BN_CONST]) == _f32(1.0 / EPS ** 0.5) and float(mean.t[T.BN_CONST]) == 3.0
    m, s = mean.t.cpu(), invstd.t.cpu()
    out = _Buf(N, C, HW)
    _call('frtm_bn_apply_relu', xd, mean.t, invstd.t, _d(d['gamma']), _d(d['beta']), N, C, HW, out.t)
    o64, o32 = _legs(T.bn_apply_relu, d['x'], m, s, d['gamma'], d['beta'])
    _check('k_bn_apply_relu', case, out.done(), o64, o32)
    return m, s, out.t.cpu()


def _bn_backward(d, N, C, HW, train, m, s, out, affine=True):
    dx, dg, db, part = _Buf(N, C, HW), _Buf(C), _Buf(C), _part(N, C, 3)
    _call('frtm_bn_relu_backward', _d(d['dy']), _d(out), _d(d['x']), _d(m), _d(s), _d(d['gamma']), N, C, HW, train, dx.t,
          dg.t if affine else None, db.t if affine else None, part.t)
    part.done()
    return dx, dg, db


@pytest.mark.parametrize('mode', BN_MODES, ids=lambda m_: m_[0].replace(' ', '_'))
@pytest.mark.parametrize('N,C,HW', T.BN_SIZES)
def test_batchnorm_relu(N, C, HW, mode):
    name, train, factor, running, with_part = mode
    d = T.bn_inputs(N, C, HW)
    case = 'N%d C%d HW%d %s' % (N, C, HW, name)
    m, s, out = _bn_forward(d, N, C, HW, train, factor, running, with_part, case)
    dx, dg, db = _bn_backward(d, N, C, HW, train, m, s, out)
    r64, r32 = _legs(lambda dy_, o_, x_, m_, s_, g_: T.bn_relu_backward(dy_, o_, x_, m_, s_, g_, train), d['dy'], out, d['x'], m, s, d['gamma'])
    _check('k_bn_bwd_apply', 'dx ' + case, dx.done(), r64[0], r32[0])
    _check('k_bn_bwd_apply', 'dgamma ' + case, dg.done(), r64[1], r32[1])
    _check('k_bn_bwd_apply', 'dbeta ' + case, db.done(), r64[2], r32[2])
    if C > 3:
        k = T.BN_DEAD
        assert float(out[:, k].abs().max()) == 0
        assert float(dx.t[:, k].abs().max()) == 0 and float(dg.t[k]) == 0 and float(db.t[k]) == 0
    if N * C * HW >= 255:
        assert 0.3 < float((out == 0).float().mean()) < 0.7
    if name in ('train f 0.1', 'eval'):                           # without the affine gradients: the same dx, nothing else written
        dx2, dg2, db2 = _bn_backward(d, N, C, HW, train, m, s, out, affine=False)
        assert torch.equal(_bits(dx2.done()), _bits(dx.t))
        dg2.same(), db2.same()


@pytest.mark.parametrize('N,C,HW', T.BN_SIZES)
def test_batchnorm_backward_sum_dx(N, C, HW):
    """The claim in k_bn_bwd_apply: in train mode dx is formed in fp64 with one final rounding, so that per channel
        |sum dx| <= 2^-24 sum|dx| + |gamma| invstd^2 |sum g xhat| 2^-25 |mean|,
    the sums taken in float64 over the returned fp32 dx; the first term is the final rounding of each element, the second the fp32 mean (xhat is
    centred on it, not on the mean of x).  Both terms from the float64 operands; printed: the largest share of the bound per case.

    Measured on an MI355X: the largest share is 0.633, at (3,257,1), and 0.78 of the first term alone, since dx takes the mean of xhat out of
    its last term; while xhat was only centred on the fp32 mean the shares reached 1.946 (module docstring)."""
    d = T.bn_inputs(N, C, HW)
    m, s, out = _bn_forward(d, N, C, HW, 1, _f32(0.1), True, True, 'N%d C%d HW%d sum dx' % (N, C, HW))
    dx = _bn_backward(d, N, C, HW, 1, m, s, out)[0].done().double().cpu()
    x, dy, m, s, gamma = d['x'].double(), d['dy'].double(), m.double(), s.double(), d['gamma'].double()
    g = torch.where(out > 0, dy, torch.zeros_like(dy))
    gx = (g * (x - m[None, :, None]) * s[None, :, None]).sum(dim=(0, 2)).abs()
    t1, t2 = 2.0 ** -24 * dx.abs().sum(dim=(0, 2)), gamma.abs() * s ** 2 * gx * 2.0 ** -25 * m.abs()
    total = dx.sum(dim=(0, 2)).abs()
    share = total / (t1 + t2).clamp_min(1e-300)
    exact = gamma.abs() * s ** 2 * gx * (x.mean(dim=(0, 2)) - m).abs()
    k = int(share.argmax())
    print('SUMDX N%d C%d HW%d largest share %.3f (channel %d: |sum dx| %.3e, rounding term %.3e, mean term %.3e); with the measured |mean64 - '
          'mean32| in the mean term %.3f' % (N, C, HW, float(share[k]), k, float(total[k]), float(t1[k]), float(t2[k]),
                                            float((total / (t1 + exact).clamp_min(1e-300)).max())))
    assert bool((total <= t1 + t2).all()), 'channel %d: |sum dx| %.3e above %.3e + %.3e' % (k, float(total[k]), float(t1[k]), float(t2[k]))


def test_batchnorm_refusals():
    z = _d(torch.zeros(65536))
    v = _d(torch.ones(65536))
    out, part = _Buf(65536), _part(256, 256, 3)
    with pytest.raises(RuntimeError, match='frtm_bn_apply_relu: bad argument'):
        _call('frtm_bn_apply_relu', z, z, v, v, z, 256, 256, 1, out.t)
    dx, dg, db = _Buf(65536), _Buf(256), _Buf(256)
    with pytest.raises(RuntimeError, match='frtm_bn_relu_backward: bad argument'):
        _call('frtm_bn_relu_backward', z, z, z, z, v, v, 256, 256, 1, 1, dx.t, dg.t, db.t, part.t)
    mean, invstd = _Buf(65536), _Buf(65536)
    for N, C in ((65536, 1), (1, 65536)):
        with pytest.raises(RuntimeError, match='frtm_bn_stats: bad argument'):
            _call('frtm_bn_stats', z, N, C, 1, EPS, 0.1, 1, None, None, mean.t, invstd.t, part.t)
    for rm, rv in ((None, None), (v, None), (None, v)):
        with pytest.raises(RuntimeError, match='frtm_bn_stats: missing buffers'):
            _call('frtm_bn_stats', z, 2, 3, 4, EPS, 0.0, 0, rm, rv, mean.t, invstd.t, part.t)
    with pytest.raises(RuntimeError, match='frtm_bn_stats: missing buffers'):
        _call('frtm_bn_stats', z, 2, 3, 4, EPS, 0.1, 1, v, None, mean.t, invstd.t, part.t)
    with pytest.raises(RuntimeError, match='frtm_bn_stats: missing buffers'):
        _call('frtm_bn_stats', z, 2, 3, 4, EPS, 0.1, 1, None, None, mean.t, invstd.t, None)
    for b in (out, part, dx, dg, db, mean, invstd):
        b.same()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3c. input gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def _dgrad_batch(cin, k, rows, H, W):
    """2, or on the 37 x 53 map the smallest batch at which ops.wino_launch admits the 3 x 3 launch (its Cout is the gradient's channel count)."""
    from frtm_vos_amd import ops
    if (H, W) != (37, 53) or k != 3:
        return 2
    B = 2
    while not ops.wino_launch(B, H, W, rows or cin):
        B += 1
    return B


@pytest.mark.parametrize('wino', [True, False], ids=['wino', 'direct'])
@pytest.mark.parametrize('H,W', T.DGRAD_MAPS)
@pytest.mark.parametrize('cin,cout,k,rows', T.DGRAD_CONVS)
def test_conv_dgrad(cin, cout, k, rows, H, W, wino):
    from frtm_vos_amd import ops
    from frtm_vos_amd.model.refiner_train import _Runner
    from frtm_vos_amd.model.seg_network import SegNetwork
    B = _dgrad_batch(cin, k, rows, H, W)
    assert ops.wino_launch(B, H, W, rows or cin) == (k == 3 and (H, W) == (37, 53)) and B <= 16
    dy, w, res = T.dgrad_inputs(cin, cout, k, B, H, W, rows)
    net = SegNetwork(1, 8, {'layer4': 8}, False)
    net.use_winograd = wino
    R = _Runner(net, DEV)
    case = 'cin %d cout %d k %d rows %s B %d %dx%d wino %d' % (cin, cout, k, rows, B, H, W, wino)
    for residual in (None, res):
        r64, r32 = _legs(lambda dy_, w_, res_: T.conv_dgrad(dy_, w_, rows=rows, residual=res_), dy, w, residual)
        resd = _Buf(init=residual) if residual is not None else None
        got = R.dgrad(_d(dy), _d(w), residual=resd.t if resd else None, rows=rows)
        if resd:
            resd.same()
        assert not bool(torch.isnan(got).any())
        _check('dgrad', case + (' + residual' if resd else ''), got, r64, r32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3d. loss tail, scale, Adam
# ---------------------------------------------------------------------------------------------------------------------------------
BCE_SIZES = [(5, 1, 1), (5, 1, 2), (5, 1, 3), (5, 1, 5), (5, 1, 7), (130, 1, 7), (1, 260, 256)]
BCE_DEFS = [('sigmoid', 4.0, 15.0), ('with_logits', 30.0, 90.0)]


def _bce_call(z, t, N, H, W, with_dz):
    nbytes = _lib().frtm_bce_logits_workspace_bytes(N, H, W)
    assert nbytes % 8 == 0
    dz, loss, inter, uni, ws = _Buf(N, 1, H, W), _Buf(1), _IntBuf(N), _IntBuf(N), _Buf(nbytes // 4)
    _call('frtm_bce_logits', z, t, t.element_size(), N, H, W, dz.t if with_dz else None, loss.t, inter.t, uni.t, ws.t, nbytes)
    ws.guards()
    return dz, loss, inter, uni


@pytest.mark.parametrize('kind', ['u8', 'f32'])
@pytest.mark.parametrize('definition,std,clamp', BCE_DEFS)
@pytest.mark.parametrize('N,H,W', BCE_SIZES)
def test_bce_logits_edges(N, H, W, definition, std, clamp, kind):
    shape = (N, 1, H, W)
    z, t = _logits(shape, std, clamp, seed=N + H * W), _targets(shape, kind, seed=N + W)
    with torch.enable_grad():
        legs = []
        for zz, tt in ((z.double().requires_grad_(), t.double()), (_d(z).requires_grad_(), _d(t.float()))):
            loss = T.bce(zz, tt, definition)
            loss.backward()
            legs.append((loss.detach().reshape(1), zz.grad))
    zd, td = _Buf(init=z), _d(t)
    assert td.data_ptr() % 16 == 0
    dz, loss, inter, uni = _bce_call(zd.t, td, N, H, W, True)
    case = '%s N%d HW%d %s' % (definition, N, H * W, kind)
    _check('k_bce_logits', 'loss ' + case, loss.done(), legs[0][0], legs[1][0])
    _check('k_bce_logits', 'dz ' + case, dz.done(), legs[0][1], legs[1][1])
    p, g = z.double() > 0, t.double() > 0.5
    assert inter.done() == (p & g).flatten(1).sum(1).tolist() and uni.done() == (p | g).flatten(1).sum(1).tolist()
    dz2, loss2, inter2, uni2 = _bce_call(zd.t, td, N, H, W, False)              # no gradient requested: the same loss and counts, dz not written
    dz2.same(), zd.same()
    assert torch.equal(_bits(loss2.done()), _bits(loss.t)) and inter2.done() == inter.done() and uni2.done() == uni.done()


@pytest.mark.parametrize('n', [0, 1, 3, 4, 5, 1027, 2048 * 256 * 4 + 7])
def test_scale_by(n):
    x = torch.randn(n, generator=T.gen(n, 7))
    a = _d(torch.tensor([_f32(0.37)]))
    buf = _Buf(init=x)
    _call('frtm_scale_by', buf.buf.data_ptr() + 4 * GUARD, n, a)                 # (an empty view has no data_ptr of its own)
    buf.guards()
    assert torch.equal(_bits(buf.t), _bits(T.scale_by(_d(x), a)))
    if n:
        assert not torch.equal(_bits(buf.t), _bits(buf.before))


ADAM_LENGTHS = [1, 3, 2047, 2048, 2049, 4100]
ADAM_BIG = 2049 * 2048 + 5
LR, B1, B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8


class _AdamTensor:
    """p, m, v, vmax (and a plain g) of one tensor on the device; skew 1: every array starts one float past a 16-byte boundary (vec = 0)."""

    def __init__(self, n, skew, key):
        g = T.gen(n, skew, key)
        self.n, self.skew = n, skew
        self.init = dict(p=torch.randn(n, generator=g), m=torch.randn(n, generator=g) * 0.1, v=torch.rand(n, generator=g) * 0.01,
                         vmax=torch.rand(n, generator=g) * 0.02)
        self.grads = [torch.randn(n, generator=g) * s for s in (1.0, 0.1, 3.0)]
        self.bufs = {k: _Buf(init=torch.cat([torch.zeros(skew), v])) for k, v in self.init.items()}
        self.gbuf = torch.zeros(n + 4, device=DEV)

    def view(self, k):
        return self.bufs[k].t[self.skew:]

    def gview(self):
        return self.gbuf[self.skew:self.skew + self.n]

    def row(self):
        ptrs = [self.view('p').data_ptr(), self.gview().data_ptr(), self.view('m').data_ptr(), self.view('v').data_ptr(), self.view('vmax').data_ptr()]
        assert all(q % 16 == 4 * self.skew for q in ptrs)
        return ptrs + [self.n, 0 if self.skew else 1, 0]


@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('amsgrad', [True, False])
def test_adam_table(amsgrad, wd):
    tens = [_AdamTensor(n, 0, 1) for n in ADAM_LENGTHS] + [_AdamTensor(n, 1, 2) for n in ADAM_LENGTHS] + [_AdamTensor(ADAM_BIG, 0, 3)]
    unnamed = _AdamTensor(100, 0, 4)                              # in the tensor table, in no chunk
    table = tens + [unnamed]
    ntens = len(table)
    chunk = _lib().frtm_adam_chunk_elems()
    assert chunk == 2048
    chunks = [(i, c) for i, t in enumerate(tens) for c in range(-(-t.n // chunk))]
    chunks[5:5] = [(-1, 0)]
    chunks[40:40] = [(ntens, 0), (0, 5)]                          # tensor 0 has one element: chunk 5 lies beyond it
    chunks.append((2, 1))                                         # 2047 elements: chunk 1 starts at 2048
    assert len(chunks) > 2048 + 4 and len(chunks) >= ntens
    td = _d(torch.tensor([t.row() for t in table], dtype=torch.int64))
    cd = _d(torch.tensor(chunks, dtype=torch.int32))
    ref = [[{k: v.double() for k, v in t.init.items()}, {k: _d(v) for k, v in t.init.items()}] for t in tens]
    for step in (1, 2, 3):
        for t in table:
            t.gview().copy_(t.grads[step - 1])
        _call('frtm_adam_amsgrad', td, ntens, cd, len(chunks), LR, 1 - B1 ** step, 1 - B2 ** step, B1, B2, ADAM_EPS, wd, int(amsgrad))
        for t, legs in zip(tens, ref):
            for leg, gr in zip(legs, (t.grads[step - 1].double(), _d(t.grads[step - 1]))):
                leg['p'], leg['m'], leg['v'], leg['vmax'] = T.adam_step(leg['p'], gr, leg['m'], leg['v'], leg['vmax'], step, LR, B1, B2, ADAM_EPS,
                                                                        wd, amsgrad)
    for b in unnamed.bufs.values():
        b.same()
    for t, (r64, r32) in zip(tens, ref):
        case = 'n %d vec %d ams %d wd %g' % (t.n, 1 - t.skew, amsgrad, wd)
        for k in ('p', 'm', 'v', 'vmax'):
            if k == 'vmax' and not amsgrad:
                t.bufs[k].same()
                continue
            t.bufs[k].guards()
            if t.skew:
                assert float(t.bufs[k].t[0]) == 0.0, 'write below an unaligned tensor'
            _check('k_adam', '%s %s' % (k, case), t.view(k), r64[k], r32[k])
            assert k == 'vmax' or not torch.equal(_bits(t.view(k)), _bits(_d(t.init[k])))
        assert torch.equal(t.gview().cpu(), t.grads[2])


def test_adam_refusals():
    t = _AdamTensor(8, 0, 5)
    td, cd = _d(torch.tensor([t.row()], dtype=torch.int64)), _d(torch.tensor([(0, 0)], dtype=torch.int32))
    with pytest.raises(RuntimeError, match='frtm_adam_amsgrad: null table'):
        _call('frtm_adam_amsgrad', None, 1, cd, 1, LR, 0.1, 0.001, B1, B2, ADAM_EPS, 0.0, 1)
    with pytest.raises(RuntimeError, match='frtm_adam_amsgrad: 1 tensors in 0 chunks'):
        _call('frtm_adam_amsgrad', td, 1, cd, 0, LR, 0.1, 0.001, B1, B2, ADAM_EPS, 0.0, 1)
    with pytest.raises(RuntimeError, match='frtm_adam_amsgrad: bias corrections must be positive'):
        _call('frtm_adam_amsgrad', td, 1, cd, 1, LR, 0.0, 0.001, B1, B2, ADAM_EPS, 0.0, 1)
    for b in t.bufs.values():
        b.same()
