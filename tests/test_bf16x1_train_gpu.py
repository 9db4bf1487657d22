"""The bf16x1 refiner training mode on the GPU: the bf16 weight-gradient kernel (csrc/conv_wgrad_bf16x1.hip) exactly on bf16-representable data,
its rounding (to nearest even, on both operands), the locality of a NaN / Inf, a derived error bound on realistic data, determinism, the argument
checks, SegNetwork.forward_train under train_precision = 'bf16x1' and a TrainerModel run with such a refiner.

Exact cases: operands are integers in [-15, 15] (bf16 holds 8 significant bits), so every product is an integer of magnitude at most 225 and every
partial sum over the B*H*W pixels an integer below 2^24 (asserted per shape): exact in fp32 in any order.  dW and dbias must equal the fp64
gradient BIT FOR BIT.  Buffers are framed: NaN-filled outputs and workspace between sentinel bands, NaN-framed inputs.

The mode is defined by its arithmetic (sections 1-6).  The network test holds the size of the mode's effect on every parameter gradient to that of
a CPU emulation of the same roundings; the TrainerModel test prints the loss next to the fp32 one and gates on plumbing only."""
import copy
import ctypes
from collections import OrderedDict

import pytest
import torch
from torch.nn import functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = 'cuda'
GUARD = 256                   # floats of guard band on each side
SENT = 0x7FA5A5A5             # sentinel word (a NaN pattern no kernel produces)
# the plan of csrc/conv_wgrad_bf16x1.hip (wgrad_plan): 4 x 32 pixel tiles, 64 x 32 channel tiles, tiles per split = ceil(tiles x channel tiles / (256 rounds)),
# rounds = ceil(tiles x channel tiles / (256 x 32)), two slabs (one per wave pair) per split
TILE_H, TILE_W, TILE_CO, TILE_CI, TARGET, MAX_TILES = 4, 32, 64, 32, 256, 32


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """The network tests need autograd; other GPU test modules switch grad mode off process-wide."""
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    yield
    torch.set_grad_enabled(prev)


def _lib():
    from frtm_vos_amd import _hip as H
    return H.lib()


def _count():
    return _lib().frtm_conv_wgrad_bf16x1_launches()


def _count3():
    return _lib().frtm_conv_bf16x1_3x3_launches()


def plan(B, cout, cin, h, w):
    """(tiles, tiles per split, splits) as the library plans them."""
    tiles = B * ((h + TILE_H - 1) // TILE_H) * ((w + TILE_W - 1) // TILE_W)
    ct = ((cin + TILE_CI - 1) // TILE_CI) * ((cout + TILE_CO - 1) // TILE_CO)
    rounds = -(-tiles * ct // (TARGET * MAX_TILES))
    tps = -(-tiles * ct // (TARGET * rounds))
    return tiles, tps, (tiles + tps - 1) // tps


class Framed:
    """n floats between two guard bands of sentinel words."""

    def __init__(self, n, guard_value=None):
        self.n = n
        self.buf = torch.empty(n + 2 * GUARD, device=DEV)
        if guard_value is None:
            self.buf.view(torch.int32).fill_(SENT)
        else:
            self.buf.fill_(guard_value)
        self.view = self.buf[GUARD:GUARD + n]

    def intact(self):
        b = self.buf.view(torch.int32)
        return bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + self.n:] == SENT).all())


def _nan_framed(t):
    """t (CPU) copied onto the device between two NaN bands: a read past its end (instead of zero padding) shows as NaN."""
    f = Framed(t.numel(), guard_value=float('nan'))
    f.view.copy_(t.reshape(-1))
    return f.view.view(t.shape)


def _ints(g, shape):
    v = torch.randint(-15, 16, shape, generator=g).float()
    return v * (torch.rand(shape, generator=g) < 0.8).float()


def _launch(dy, x, weight=True, bias=True):
    """One framed frtm_conv_wgrad_bf16x1 call on CPU operands -> (dW, dbias) on the CPU in fp64 (None where not asked for); asserts the counter, the
    guard bands of both outputs and the workspace, and that the workspace is exactly the plan's."""
    from frtm_vos_amd import _hip as H
    L = _lib()
    B, cout, h, w = dy.shape
    cin = x.shape[1]
    elems = L.frtm_conv_wgrad_bf16x1_ws_elems(B, cout, cin, h, w)
    assert elems == 2 * plan(B, cout, cin, h, w)[2] * cout * (9 * cin + 1)
    ws = Framed(elems)
    dw, db = Framed(cout * cin * 9), Framed(cout)
    dw.view.fill_(float('nan'))
    db.view.fill_(float('nan'))
    n0, n3 = _count(), _count3()
    dyd, xd = _nan_framed(dy.float()), _nan_framed(x.float())          # (held until the synchronize below)
    H.call('frtm_conv_wgrad_bf16x1', H.ptr(dyd), H.ptr(xd), B, cout, cin, h, w,
           dw.view.data_ptr() if weight else None, db.view.data_ptr() if bias else None, ws.view.data_ptr(), elems)
    assert _count() == n0 + 1 and _count3() == n3
    torch.cuda.synchronize()
    assert dw.intact() and db.intact() and ws.intact(), 'guard band overwritten'
    gw, gb = dw.view.view(cout, cin, 3, 3).cpu().double(), db.view.cpu().double()
    if not weight:
        assert bool(torch.isnan(gw).all())                # untouched
    if not bias:
        assert bool(torch.isnan(gb).all())
    return (gw if weight else None), (gb if bias else None)


def _ref(dy, x):
    cout, cin = dy.shape[1], x.shape[1]
    return torch.nn.grad.conv2d_weight(x.double(), (cout, cin, 3, 3), dy.double(), padding=1), dy.double().sum((0, 2, 3))


def _assert_same(got, ref, label):
    assert not torch.isnan(got).any(), ('unwritten (NaN) outputs: %d' % int(torch.isnan(got).sum()),) + label
    bad = got != ref
    assert not bad.any(), ('%d of %d outputs differ, max |err| %g' % (int(bad.sum()), bad.numel(), float((got - ref).abs().max())),) + label


def wgrad_case(B, cin, cout, h, w, weight=True, bias=True, seed=0):
    assert B * h * w * 225 < 2 ** 24                       # every partial sum is an integer below 2^24: exact in fp32 in any order
    g = torch.Generator().manual_seed(seed * 7919 + B * 1009 + cin * 101 + cout * 11 + h + w)
    dy, x = _ints(g, (B, cout, h, w)), _ints(g, (B, cin, h, w))
    gw, gb = _launch(dy, x, weight, bias)
    rw, rb = _ref(dy, x)
    if weight:
        _assert_same(gw, rw, ('dW', B, cin, cout, h, w))
    if bias:
        _assert_same(gb, rb, ('dbias', B, cin, cout, h, w))


# ---- 1. exact cases
SPLIT_SHAPE = (1, 64, 64, 2081, 9)      # 521 tiles x 2 channel tiles: 5 tiles per split, 105 splits, the last one a single tile


@pytest.mark.parametrize('B,cin,cout,h,w', [
    (2, 65, 65, 9, 11),        # both channel tails, ragged in both directions
    (1, 16, 64, 19, 70),       # several tiles in both directions: interior halos
    (16, 64, 64, 15, 27),      # the deepest map of a step: a tile must never take a neighbouring image for padding
    (2, 3, 5, 1, 7),           # H = 1
    (1, 24, 80, 5, 1),         # W = 1
    (1, 1, 1, 3, 3),           # smallest everything
    (3, 64, 32, 8, 8),         # Cout 32, the head conv's output width
    SPLIT_SHAPE,               # several tiles per split and a ragged last split
])
def test_exact_shapes(B, cin, cout, h, w):
    wgrad_case(B, cin, cout, h, w)


def test_the_split_shape_has_several_splits_and_a_ragged_last_one():
    B, cin, cout, h, w = SPLIT_SHAPE
    tiles, tps, nsplit = plan(B, cout, cin, h, w)
    assert (tiles, tps, nsplit) == (521, 5, 105) and tiles % tps == 1
    assert _lib().frtm_conv_wgrad_bf16x1_ws_elems(B, cout, cin, h, w) == 2 * 105 * cout * (9 * cin + 1)
    assert plan(16, 64, 64, 15, 27)[1:] == (1, 64) and plan(1, 1, 1, 3, 3)[1:] == (1, 1)


def test_exact_weight_only_and_bias_only():
    wgrad_case(2, 65, 65, 9, 11, bias=False, seed=1)
    wgrad_case(2, 65, 65, 9, 11, weight=False, seed=2)


def test_wrapper_matches_the_entry_point_and_fp32_stays_fp32():
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(3)
    dy, x = _ints(g, (2, 40, 9, 37)), _ints(g, (2, 33, 9, 37))
    gw, gb = _launch(dy, x)
    n0 = _count()
    dw, db = ops.conv_wgrad(dy.to(DEV), x.to(DEV), 3, bf16x1=True)
    assert _count() == n0 + 1
    assert torch.equal(dw.cpu().double(), gw) and torch.equal(db.cpu().double(), gb)
    ops.conv_wgrad(dy.to(DEV), x.to(DEV), 3)
    ops.conv_wgrad(dy.to(DEV), x.to(DEV), 1)
    assert _count() == n0 + 1                             # the fp32 path does not move the counter


# ---- 2. rounding: to nearest even, on both operands
RNE_VALUES = (1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -7 - 2.0 ** -20, 1.5 + 2.0 ** -9)
RNE_ROUNDED = (1.0, 1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1 + 2.0 ** -7, 1.5)      # ties (entries 1-3) go to the even neighbour


def _truncated(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


@pytest.mark.parametrize('which', ('x', 'dy'))
def test_operands_are_rounded_to_nearest_even(which):
    """dY is one-hot per output channel: one pixel of one image.  dW[co, ci, kh, kw] is then ONE product, dy[co] * x[n, ci, y - 1 + kh, x - 1 + kw],
    exact in fp32 (two 8-bit significands), and dbias[co] the rounded dy[co].  First x is drawn from RNE_VALUES (dy +-1), then dy (x +-1, +-2)."""
    B, cin, cout, h, w = 2, 65, 72, 9, 37
    g = torch.Generator().manual_seed(17)
    vals = torch.tensor(RNE_VALUES, dtype=torch.float64)
    assert torch.equal(torch.tensor(RNE_VALUES, dtype=torch.float32).bfloat16().double(), torch.tensor(RNE_ROUNDED, dtype=torch.float64))

    def draw(shape):
        v = vals[torch.randint(0, len(RNE_VALUES), shape, generator=g)]
        return (v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()
    hot = torch.zeros(B, cout, h, w)
    m = torch.arange(cout)
    hot[m % B, m, (m * 5) % h, (m * 7) % w] = 1.0            # every row and both tiles of columns, the corners' paddings included
    if which == 'x':
        x = draw((B, cin, h, w))
        dy = hot * (torch.randint(0, 2, (1, cout, 1, 1), generator=g) * 2 - 1).float()
    else:
        x = (torch.randint(1, 3, (B, cin, h, w), generator=g) * (torch.randint(0, 2, (B, cin, h, w), generator=g) * 2 - 1)).float()
        dy = hot * draw((1, cout, 1, 1))
    rw, rb = _ref(dy.bfloat16(), x.bfloat16())
    assert torch.equal(rw.float().double(), rw)
    tw, tb = _ref(_truncated(dy), _truncated(x))
    assert not (torch.equal(tw, rw) and torch.equal(tb, rb))          # the data discriminates: truncation ...
    nw, nb = _ref(dy, x)
    assert not (torch.equal(nw, rw) and torch.equal(nb, rb))          # ... or no rounding at all gives another result somewhere
    gw, gb = _launch(dy, x)
    _assert_same(gw, rw, ('dW', which))
    _assert_same(gb, rb, ('dbias', which))
    assert not torch.equal(gw, tw) or not torch.equal(gb, tb)


# ---- 3. NaN / Inf locality
@pytest.mark.parametrize('value', (float('nan'), float('inf')))
def test_a_nan_in_dy_taints_its_row_only(value):
    B, cin, cout, h, w = 2, 65, 66, 7, 37
    g = torch.Generator().manual_seed(43)
    dy, x = _ints(g, (B, cout, h, w)), torch.randint(1, 8, (B, cin, h, w), generator=g).float()      # x all positive
    cw, cb = _launch(dy, x)
    for co, py, px in ((0, 0, 0), (65, 6, 36), (33, 3, 31)):
        d = dy.clone()
        d[1, co, py, px] = value
        gw, gb = _launch(d, x)
        rows = torch.zeros(cout, dtype=torch.bool)
        rows[co] = True
        if value != value:
            assert bool(torch.isnan(gw[co]).all()) and bool(torch.isnan(gb[co]))
        else:                                                        # Inf x positive = Inf where the tap reads the map, Inf x 0 = NaN in the padding
            assert bool((torch.isinf(gw[co]) | torch.isnan(gw[co])).all()) and bool(torch.isinf(gw[co, :, 1, 1]).all()) and bool(torch.isinf(gb[co]))
        assert torch.equal(gw[~rows], cw[~rows]) and torch.equal(gb[~rows], cb[~rows]), (co, py, px)


@pytest.mark.parametrize('chan', (0, 64))                                     # the first tile, and the tail tile of Cin = 65
@pytest.mark.parametrize('py,px', [(0, 0), (6, 36), (0, 31), (3, 32), (6, 4), (3, 17)])   # corners, edges, both sides of a tile border, the interior
def test_a_nan_in_x_taints_exactly_the_taps_that_read_it(py, px, chan):
    """W = 37: the second tile of columns overhangs the image by 27 pixel slots, whose dY is zero but whose left neighbour (column 36) is real."""
    B, cin, cout, h, w = 2, 65, 8, 7, 37
    g = torch.Generator().manual_seed(41 + py * 9 + px + chan)
    x = _ints(g, (B, cin, h, w))
    dy = torch.randint(1, 8, (B, cout, h, w), generator=g).float()            # all positive
    cw, cb = _launch(dy, x)
    want = torch.zeros(cout, cin, 3, 3, dtype=torch.bool)
    for kh in range(3):
        for kw in range(3):
            if 0 <= py + 1 - kh < h and 0 <= px + 1 - kw < w:                 # the output pixel whose tap (kh, kw) reads x[py, px]
                want[:, chan, kh, kw] = True
    for value in (float('nan'), float('inf')):
        xv = x.clone()
        xv[1, chan, py, px] = value
        gw, gb = _launch(dy, xv)
        hit = torch.isnan(gw) if value != value else (gw == float('inf'))
        assert torch.equal(hit, want), (value, int(hit.sum()), int(want.sum()))
        assert torch.equal(gw[~want], cw[~want]) and torch.equal(gb, cb), value


# ---- 4. error bound on realistic data
@pytest.mark.parametrize('B,cin,cout,h,w', [(2, 64, 64, 30, 54), (2, 65, 65, 24, 40), (1, 64, 32, 48, 60)])
def test_error_within_the_derived_bound(B, cin, cout, h, w):
    """|dW - fp64| <= (2^-7 + 2^-16 + L 2^-22) (|dY| (x) |X|) element-wise and |dbias - fp64| <= (2^-8 + L 2^-22) sum |dY|: (2u + u^2), u = 2^-8, for
    the two operand roundings (u for the bias: 1.0 is exact), L 2^-22 for L fp32 accumulations with the factor 4 over round-to-nearest of the other
    bf16x1 bounds.  L from the kernel's constants: a wave adds its two rows of 32 pixels of each of a split's tiles to ONE accumulator, a split
    has at most MAX_TILES = 32 tiles, so a chain is at most 32 x 64 = 2048 pixels long; the chains' slabs are summed in fp64 (exact at this
    size) and rounded to fp32 once: L = 2048 + 1.  Derived, not measured."""
    from frtm_vos_amd import ops
    L = MAX_TILES * 2 * TILE_W + 1
    assert plan(B, cout, cin, h, w)[1] <= MAX_TILES
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.relu(torch.randn(B, cin, h, w, generator=g))
    dy = torch.randn(B, cout, h, w, generator=g)
    rw, rb = _ref(dy, x)
    magw, magb = _ref(dy.abs(), x.abs())
    n0 = _count()
    dw, db = ops.conv_wgrad(dy.to(DEV), x.to(DEV), 3, bf16x1=True)
    assert _count() == n0 + 1
    ew, eb = (dw.cpu().double() - rw).abs(), (db.cpu().double() - rb).abs()
    bw, bb = (2.0 ** -7 + 2.0 ** -16 + L * 2.0 ** -22) * magw, (2.0 ** -8 + L * 2.0 ** -22) * magb
    print('%d->%d %dx%dx%d: dW max err %.3e, worst err / bound %.3f; dbias max err %.3e, worst err / bound %.3f' % (
        cin, cout, B, h, w, float(ew.max()), float((ew / bw.clamp_min(1e-30)).max()), float(eb.max()), float((eb / bb.clamp_min(1e-30)).max())))
    assert bool((ew <= bw).all()) and bool((eb <= bb).all())
    assert float(ew.max()) > 1e-5                                           # the launch really rounded its operands


# ---- 5. determinism
def test_two_calls_are_bit_identical():
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(23)
    dy, x = torch.randn(4, 80, 13, 37, generator=g).to(DEV), torch.randn(4, 65, 13, 37, generator=g).to(DEV)
    n0 = _count()
    a = ops.conv_wgrad(dy, x, 3, bf16x1=True)
    b = ops.conv_wgrad(dy, x, 3, bf16x1=True)
    assert _count() == n0 + 2
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ops.conv_wgrad(dy, x, 3)
    assert _count() == n0 + 2


# ---- 6. argument checks
def test_refusals():
    from frtm_vos_amd import ops
    L = _lib()
    t = torch.zeros(1 << 16, device=DEV)
    p = ctypes.c_void_p(t.data_ptr())
    elems = L.frtm_conv_wgrad_bf16x1_ws_elems(1, 8, 8, 8, 8)
    assert 0 < elems <= t.numel()
    n0 = _count()
    for args in ((None, p, 1, 8, 8, 8, 8, p, p, p, elems), (p, None, 1, 8, 8, 8, 8, p, p, p, elems), (p, p, 1, 8, 8, 8, 8, None, None, p, elems),
                 (p, p, 1, 8, 8, 8, 8, p, p, None, elems), (p, p, 0, 8, 8, 8, 8, p, p, p, elems), (p, p, 1, 8, 8, 0, 8, p, p, p, elems),
                 (p, p, 1, 8, 8, 8, 8, p, p, p, elems - 1), (p, p, 1, 8, 8, 8, 8, p, p, p, 0)):
        assert L.frtm_conv_wgrad_bf16x1(*args, None) == -1, args
        assert b'frtm_conv_wgrad_bf16x1' in L.frtm_last_error()
    x = torch.zeros(1, 8, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.conv_wgrad(x, x, 1, bf16x1=True)                  # the bf16x1 form is a 3x3 gradient: no launch of either kernel
    assert _count() == n0


# ---- 7. network
SMALL = OrderedDict(layer5=32, layer4=16, layer3=8, layer2=8)


def _net(chans, seed=1):
    from frtm_vos_amd.model.seg_network import SegNetwork
    torch.manual_seed(seed)
    net = SegNetwork(1, 64, chans, True)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for name, b in net.named_buffers():
            if name.endswith('running_var'):
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)
            elif name.endswith('running_mean'):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
        for name, p in net.named_parameters():
            if name.endswith('bias'):
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return net


def _inputs(chans, B, Hh, Ww, seed=2):
    g = torch.Generator().manual_seed(seed)
    feats = {}
    for i, (L, c) in enumerate(chans.items()):
        s = 32 >> i
        feats[L] = torch.relu(torch.randn(B, c, (Hh + s - 1) // s, (Ww + s - 1) // s, generator=g))
    scores = torch.randn(B, 1, feats['layer4'].shape[2], feats['layer4'].shape[3], generator=g)
    return scores, feats


class _Bf16Conv3x3(torch.autograd.Function):
    """The mode's roundings on the CPU: (x, w) rounded for the output, (dy, w) for the input gradient, (dy, x) for the weight gradient; the bias
    gradient is the sum of the rounded dy (the ones column)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        return F.conv2d(x.bfloat16().float(), w.bfloat16().float(), b, 1, 1)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        d = dy.bfloat16().float()
        dx = torch.nn.grad.conv2d_input(x.shape, w.bfloat16().float(), d, padding=1)
        dw = torch.nn.grad.conv2d_weight(x.bfloat16().float(), w.shape, d, padding=1)
        return dx, dw, d.sum((0, 2, 3)) if ctx.has_bias else None


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def test_network_under_train_precision_bf16x1():
    B, Hh, Ww = 2, 96, 160
    cpu = _net(SMALL).train()
    scores, feats = _inputs(SMALL, B, Hh, Ww)
    dl = torch.randn(B, 1, Hh, Ww, generator=torch.Generator().manual_seed(9))

    def run(net, sc, ft, d, hip):
        bufs = {k: b.clone() for k, b in net.named_buffers()}
        for p in net.parameters():
            p.grad = None
        out = net.forward_train(sc, ft, (Hh, Ww)) if hip else net.forward_torch(sc, ft, (Hh, Ww))
        out.backward(d)
        with torch.no_grad():
            for k, b in net.named_buffers():
                b.copy_(bufs[k])                              # the same running statistics for every run
        return out.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}

    _, g_ref = run(copy.deepcopy(cpu), scores, feats, dl, False)
    emu = copy.deepcopy(cpu)
    for m in emu.modules():                                   # (the head's conv2 runs in the fused tail and on the tap maps: fp32 in the mode too)
        if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m is not emu.project.conv2:
            m.forward = (lambda mod: lambda t: _Bf16Conv3x3.apply(t, mod.weight, mod.bias))(m)
    _, g_emu = run(emu, scores, feats, dl, False)

    net = copy.deepcopy(cpu).to(DEV).train()
    assert net.train_precision == 'fp32'
    net.bf16_min_blocks = 0
    sc, ft, d = scores.to(DEV), {k: v.to(DEV) for k, v in feats.items()}, dl.to(DEV)

    def hip():
        a, b = _count3(), _count()
        out, g = run(net, sc, ft, d, True)
        torch.cuda.synchronize()
        return out, g, _count3() - a, _count() - b
    o1, g1, n3, nw = hip()
    assert n3 == 0 and nw == 0                                # (a) neither counter moves under fp32
    net.train_precision = 'bf16x1'
    ob, gb, n3, nw = hip()
    assert n3 > 0 and nw > 0, (n3, nw)                        # (a) both move under bf16x1
    # 8 3x3 convs per level (transform[0], [2], [4], four RRB convs ... ) + the head's conv1: one weight gradient each
    assert nw == sum(1 for m in net.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3) and m is not net.project.conv2), nw
    ob2, gb2, n3b, nwb = hip()
    assert (n3b, nwb) == (n3, nw) and torch.equal(ob, ob2)
    for k in gb:
        assert torch.equal(gb[k], gb2[k]), k                  # (c) two bf16x1 runs are bit-identical
    net.train_precision = 'fp32'
    o3, g3, n3, nw = hip()
    assert n3 == 0 and nw == 0 and torch.equal(o1, o3)
    for k in g1:
        assert torch.equal(g1[k], g3[k]), k                   # (b) fp32 before and after the switch: bit-identical
    # (d) the size of the effect, per parameter
    assert set(gb) == set(g_ref) == set(g_emu)
    worst = 0.0
    for k in g_ref:
        e = _rms(g_emu[k] - g_ref[k])
        dk = _rms(gb[k].cpu() - g1[k].cpu())
        if k.endswith('bblock.0.bias'):                       # analytically zero under batch statistics: rounding noise on both sides
            floor = 1e-5 * float(g_ref[k.replace('bias', 'weight')].abs().max())
            assert dk <= max(3 * e, floor), (k, dk, e, floor)
            continue
        if e > 0:
            worst = max(worst, dk / e)
            assert 0 < dk <= 3 * e, (k, dk, e)
        else:
            assert dk == 0, (k, dk)
    print('worst d_k / e_k over %d parameters: %.3f; logits rms %.3e, bf16x1 - fp32 logits rms %.3e' % (len(g_ref), worst, _rms(o1), _rms(ob - o1)))


# ---- 8. TrainerModel plumbing
def test_trainer_model_runs_with_a_bf16x1_refiner(tmp_path):
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    from frtm_vos_amd.model.augmenter import ImageAugmenter
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    from frtm_vos_amd.model.seg_network import SegNetwork
    from frtm_vos_amd.model.training_model import SampleSpec, TrainerModel
    P = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18')
    P.disc_params.update(memory_size=20, init_iters=(3, 5), update_iters=(3,), c_channels=32)
    ext = ResnetFeatureExtractor('resnet18').to(DEV)
    chans = {L: n for L, n in ext.get_out_channels().items() if L in P.refnet_params.layers}
    seqs = [SyntheticSequence('s%d' % k, 3, (128, 160), 1, seed=30 + k) for k in range(2)]
    images = [torch.stack([s.images[t] for s in seqs]) for t in range(3)]
    labels = [torch.stack([(s.gt[t] == 1).to(torch.uint8) for s in seqs]) for t in range(3)]
    meta = [SampleSpec('s%d' % k, 1, ['00000', '00001', '00002'], 0).encoded() for k in range(2)]
    first = {}
    for mode in ('fp32', 'bf16x1'):
        torch.manual_seed(1)
        refiner = SegNetwork(1, 64, chans, True, train_precision=mode).to(DEV)
        refiner.bf16_min_blocks = 0                           # the maps of 128x160 frames are below any measured rule's sizes
        m = TrainerModel(ImageAugmenter(P.aug_params), ext, P.disc_params, refiner, batch_size=2,
                         tmodel_cache=dict(path=tmp_path / 'cache', enable=True, read_only=False), device=DEV, refiner_backend='hip')
        __import__('numpy').random.seed(0)
        opt = torch.optim.Adam(refiner.parameters(), lr=1e-3)
        a3, aw = _count3(), _count()
        losses = []
        for step in range(2):
            opt.zero_grad()
            losses.append(float(m(images, labels, meta)['stats/loss']))
            assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in refiner.parameters())
            opt.step()
        torch.cuda.synchronize()
        moved = (_count3() - a3, _count() - aw)
        assert all(v == v and abs(v) != float('inf') for v in losses), losses
        assert (moved[0] > 0 and moved[1] > 0) if mode == 'bf16x1' else moved == (0, 0), (mode, moved)
        first[mode] = losses[0]
    print('first-step loss: fp32 %.6f, bf16x1 %.6f (not gated)' % (first['fp32'], first['bf16x1']))
