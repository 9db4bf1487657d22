"""The bf16x1 refiner mode on the GPU: the FRTM_WLAYOUT_BF16X1_3X3 kernel (csrc/conv3x3_bf16x1.hip) exactly on bf16-representable data, its rounding
(to nearest even, on both operands), the locality of a NaN / Inf, a derived error bound on realistic data, determinism across launches, batches and
tile forms, the argument checks, the refiner's routing and a tracker run with a bf16x1 refiner.

Exact cases: operands are integers in [-15, 15] (bf16 holds 8 significant bits), so every product and every partial sum of up to 9 x 72 of them is an
integer below 2^24 and exact in fp32 in any order; the epilogue (scale +-{0.5, 1, 2}, quarter-step shift and residual) keeps that.  The output must
equal an fp64 convolution BIT FOR BIT.  Buffers are framed: NaN-filled outputs between sentinel bands, NaN-framed inputs and residuals.

The mode is defined by its arithmetic (sections 1-5).  The refiner test holds the size of the mode's effect on the logits to that of a CPU emulation
of the same roundings; the tracker test prints the label agreement and gates on plumbing only."""
import copy
import ctypes
import itertools

import pytest
import torch
from torch.nn import functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = 'cuda'
BF16X1, BF16X1_3X3 = 6, 7
TILES = (0, 1, 2)             # frtm_conv_desc.tile: automatic, FRTM_BF16X1_3X3_TILE_64, FRTM_BF16X1_3X3_TILE_96
KERNEL = {1: 'k_conv3x3_bf16x1<2>', 2: 'k_conv3x3_bf16x1<3>'}
GUARD = 256                   # floats of guard band on each side (a multiple of 4: the framed tensors keep 16-byte alignment)
SENT = 0x7FA5A5A5             # sentinel word (a NaN pattern no kernel produces)


def _lib():
    from frtm_vos_amd import _hip as H
    return H.lib()


def _last():
    return _lib().frtm_conv_last_kernels().decode()


def _count():
    return _lib().frtm_conv_bf16x1_3x3_launches()


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


def _launch(x, wt, tile=0, scale=None, shift=None, residual=None, relu=False):
    """One framed FRTM_WLAYOUT_BF16X1_3X3 call on CPU operands -> the result on the CPU in fp64; asserts the kernels, the two counters and the
    guard bands, and that every output was written."""
    from frtm_vos_amd import ops
    L = _lib()
    B, cin, h, w = x.shape
    cout = wt.shape[0]
    wB, _, lay = ops.pack_weights(wt.float().to(DEV), bf16x1=True)
    assert lay == BF16X1_3X3 and _last() == 'k_pack_weights_bf16x1_3x3' and wB.numel() == ops.bf16x1_3x3_elems(cout, cin)
    out = Framed(B * cout * h * w)
    out.view.fill_(float('nan'))
    n0, n1 = _count(), L.frtm_conv_bf16x1_launches()
    ops.conv2d(_nan_framed(x.float()), wB, cout, 3, 1, 1, scale=None if scale is None else scale.float().to(DEV),
               shift=None if shift is None else shift.float().to(DEV), residual=None if residual is None else _nan_framed(residual.float()),
               relu=relu, out=out.view.view(B, cout, h, w), w_layout=BF16X1_3X3, tile=tile)
    assert _last() in KERNEL.values() and (tile == 0 or _last() == KERNEL[tile]), _last()
    assert _count() == n0 + 1 and L.frtm_conv_bf16x1_launches() == n1          # its own counter; the 1x1 counter does not move
    torch.cuda.synchronize()
    assert out.intact(), 'output guard band overwritten'
    return out.view.view(B, cout, h, w).cpu().double()


def bf_case(B, cin, cout, h, w, tile, scale=False, res=False, relu=False, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + B * 1009 + cin * 101 + cout * 11 + h + w)
    x, wt = _ints(g, (B, cin, h, w)), _ints(g, (cout, cin, 3, 3))
    sc = (2.0 ** torch.randint(-1, 2, (cout,), generator=g)) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1)
    sh = torch.randint(-8, 9, (cout,), generator=g) / 4.0
    rs = torch.randint(-8, 9, (B, cout, h, w), generator=g) / 4.0
    got = _launch(x, wt, tile, sc if scale else None, sh if scale else None, rs if res else None, relu)
    label = (B, cin, cout, h, w, tile, scale, res, relu)
    assert not torch.isnan(got).any(), ('unwritten (NaN) outputs: %d' % int(torch.isnan(got).sum()),) + label
    ref = F.conv2d(x.double(), wt.double(), padding=1)
    if scale:
        ref = ref * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    if res:
        ref = ref + rs.double()
    if relu:
        ref = torch.relu(ref)
    bad = got != ref
    assert not bad.any(), ('%d of %d outputs differ, max |err| %g' % (int(bad.sum()), bad.numel(), float((got - ref).abs().max())),) + label
    return got


# ---- 1. exact cases
@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('B,cin,cout,h,w', [
    (2, 65, 65, 9, 11),        # both channel tails, ragged in both directions
    (1, 16, 64, 19, 70),       # several tiles in both directions: interior halos
    (16, 64, 64, 15, 27),      # the window's deepest map: a tile must never take a neighbouring image for padding
    (2, 3, 5, 1, 7),           # H = 1
    (1, 24, 80, 5, 1),         # W = 1
    (1, 1, 1, 3, 3),           # smallest everything
    (3, 64, 32, 8, 8),         # Cout 32, the head conv's output width
])
def test_exact_shapes(B, cin, cout, h, w, tile):
    bf_case(B, cin, cout, h, w, tile, scale=True, res=True, relu=True)


@pytest.mark.parametrize('tile', (1, 2))
@pytest.mark.parametrize('scale,res,relu', list(itertools.product((False, True), repeat=3)))
def test_exact_every_epilogue(scale, res, relu, tile):
    bf_case(2, 72, 40, 9, 7, tile, scale=scale, res=res, relu=relu, seed=1)


def test_exact_data_is_exact_in_fp32_at_k_585():
    """The claim the exact cases rest on, on the CPU: with K = 9 x 65 = 585 operands of magnitude at most 15, every partial sum is at most
    585 x 225 < 2^24, so the fp32 sum (in torch's order) equals the fp64 sum; the largest K of the exact cases is 9 x 72 = 648."""
    assert 648 * 15 * 15 < 2 ** 24
    g = torch.Generator().manual_seed(5)
    x, wt = _ints(g, (2, 65, 9, 11)), _ints(g, (65, 65, 3, 3))
    assert torch.equal(F.conv2d(x, wt, padding=1).double(), F.conv2d(x.double(), wt.double(), padding=1))
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(wt.bfloat16().float(), wt)       # bf16-representable


# ---- 2. rounding: to nearest even, on both operands
RNE_VALUES = (1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -7 - 2.0 ** -20, 1.5 + 2.0 ** -9)
RNE_ROUNDED = (1.0, 1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1 + 2.0 ** -7, 1.5)      # ties (entries 1-3) go to the even neighbour


def _truncated(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


@pytest.mark.parametrize('tile', (1, 2))
@pytest.mark.parametrize('which', ('activations', 'weights'))
def test_operands_are_rounded_to_nearest_even(which, tile):
    """One-hot weights: output m is ONE product, w[m] * x[ci(m), y - 1 + kh(m), x - 1 + kw(m)], exact in fp32 (two 8-bit significands).  First
    the activations are drawn from RNE_VALUES (weights +-1), then the weights (activations +-1, +-2)."""
    B, cin, cout, h, w = 2, 65, 72, 9, 7
    g = torch.Generator().manual_seed(17)
    vals = torch.tensor(RNE_VALUES, dtype=torch.float64)
    assert torch.equal(torch.tensor(RNE_VALUES, dtype=torch.float32).bfloat16().double(), torch.tensor(RNE_ROUNDED, dtype=torch.float64))

    def draw(shape):
        v = vals[torch.randint(0, len(RNE_VALUES), shape, generator=g)]
        return (v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()
    hot = torch.zeros(cout, cin, 3, 3)
    m = torch.arange(cout)
    hot[m, (m * 7) % cin, m % 3, (m // 3) % 3] = 1.0                         # every tap, channels up to the tail group (64 = 7 x 46 % 65: m = 46)
    assert int(((m * 7) % cin).max()) == cin - 1
    if which == 'activations':
        x = draw((B, cin, h, w))
        wt = hot * (torch.randint(0, 2, (cout, 1, 1, 1), generator=g) * 2 - 1).float()
    else:
        x = (torch.randint(1, 3, (B, cin, h, w), generator=g) * (torch.randint(0, 2, (B, cin, h, w), generator=g) * 2 - 1)).float()
        wt = hot * draw((cout, 1, 1, 1))
    ref = F.conv2d(x.bfloat16().double(), wt.bfloat16().double(), padding=1)
    assert torch.equal(ref.float().double(), ref)
    # the data discriminates: truncation, or no rounding at all, gives another result somewhere
    assert not torch.equal(F.conv2d(_truncated(x).double(), _truncated(wt).double(), padding=1), ref)
    assert not torch.equal(F.conv2d(x.double(), wt.double(), padding=1), ref)
    got = _launch(x, wt, tile)
    assert not torch.isnan(got).any()
    bad = got != ref
    assert not bad.any(), '%d of %d outputs differ from the round-to-nearest-even product, max |err| %g' % (
        int(bad.sum()), bad.numel(), float((got - ref).abs().max()))


# ---- 3. NaN / Inf locality
@pytest.mark.parametrize('chan', (0, 64))                                     # the first group, and the tail group of Cin = 65
@pytest.mark.parametrize('py,px', [(0, 0), (6, 8), (0, 4), (3, 8), (3, 4)])   # two corners, two edges, the interior
def test_a_nan_reaches_exactly_the_windows_that_cover_it(py, px, chan):
    B, cin, cout, h, w = 2, 65, 8, 7, 9
    g = torch.Generator().manual_seed(41 + py * 9 + px + chan)
    x = _ints(g, (B, cin, h, w))
    wt = torch.randint(1, 8, (cout, cin, 3, 3), generator=g).float()          # all positive
    clean = F.conv2d(x.double(), wt.double(), padding=1)
    want = torch.zeros(B, cout, h, w, dtype=torch.bool)
    want[1, :, max(py - 1, 0):py + 2, max(px - 1, 0):px + 2] = True           # every output channel of that image, the 3x3 neighbourhood
    for tile in (1, 2):
        for value in (float('nan'), float('inf')):
            xv = x.clone()
            xv[1, chan, py, px] = value
            got = _launch(xv, wt, tile)
            hit = torch.isnan(got) if value != value else (got == float('inf'))
            assert torch.equal(hit, want), (tile, value, int(hit.sum()), int(want.sum()))
            assert torch.equal(got[~want], clean[~want]), (tile, value)


# ---- 4. error bound on realistic data
@pytest.mark.parametrize('B,cin,cout,h,w', [(2, 64, 64, 30, 54), (2, 65, 65, 24, 40), (1, 64, 32, 48, 60)])
def test_error_within_the_derived_bound(B, cin, cout, h, w):
    """|out - fp64| <= (2^-7 + 2^-16 + K 2^-22) |scale| (|W| conv |X|) element-wise with K = 9 Cin -- (2u + u^2), u = 2^-8, for the two operand
    roundings; K 2^-22 for K fp32 accumulations with a factor 4 over round-to-nearest for the MFMA's internal sum: the bound of the 1x1 form with the
    longer K -- plus the epilogue's own fp32 rounding: 2^-23 (|scale| |acc| + |value before the residual| + |value after it|), one rounding each for the
    scaling (or a fused multiply-add), the shift and the residual add, with |acc| bounded by |W| conv |X|.  Derived, not measured."""
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.relu(torch.randn(B, cin, h, w, generator=g)).to(DEV)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(DEV)
    sc = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    sh = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    rs = torch.randn(B, cout, h, w, generator=g).to(DEV)
    K = 9 * cin
    s64, h64 = sc.double().view(1, -1, 1, 1), sh.double().view(1, -1, 1, 1)
    mag = F.conv2d(x.double(), wt.double().abs(), padding=1)                  # (x >= 0)
    pre = F.conv2d(x.double(), wt.double(), padding=1) * s64 + h64
    ref = torch.relu(pre + rs.double())
    bound = (2.0 ** -7 + 2.0 ** -16 + K * 2.0 ** -22) * s64.abs() * mag + 2.0 ** -23 * (s64.abs() * mag * (1 + 2.0 ** -6) + pre.abs() + (pre + rs.double()).abs()) * (1 + 2.0 ** -6)
    wB, _, _ = ops.pack_weights(wt, bf16x1=True)
    for tile in TILES:
        got = ops.conv2d(x, wB, cout, 3, 1, 1, scale=sc, shift=sh, residual=rs, relu=True, w_layout=BF16X1_3X3, tile=tile)
        assert _last() in KERNEL.values() and (tile == 0 or _last() == KERNEL[tile])
        err = (got.double() - ref).abs()
        ratio = float((err / bound.clamp_min(1e-30)).max())
        print('%d->%d %dx%d tile %d (%s): max err %.3e, worst err / bound %.3f' % (cin, cout, h, w, tile, _last(), float(err.max()), ratio))
        assert bool((err <= bound).all()), (cin, cout, tile, ratio)
        assert float(err.max()) > 1e-5                                      # (the launch really rounded its operands: fp32 kernels sit near 1e-6 here)


# ---- 5. determinism: launches, batches, tile forms
def test_bit_identical_across_launches_batches_and_forms():
    from frtm_vos_amd import ops
    B, cin, cout, h, w = 4, 65, 80, 13, 37
    g = torch.Generator().manual_seed(23)
    x = torch.randn(B, cin, h, w, generator=g).to(DEV)
    wt = torch.randn(cout, cin, 3, 3, generator=g).to(DEV)
    rs = torch.randn(B, cout, h, w, generator=g).to(DEV)
    wB, _, _ = ops.pack_weights(wt, bf16x1=True)
    outs = {}
    for tile in TILES:
        a = ops.conv2d(x, wB, cout, 3, 1, 1, residual=rs, relu=True, w_layout=BF16X1_3X3, tile=tile)
        b = ops.conv2d(x, wB, cout, 3, 1, 1, residual=rs, relu=True, w_layout=BF16X1_3X3, tile=tile)
        assert torch.equal(a, b), tile
        for i in range(B):                                                   # B = 4 against four B = 1 calls
            c = ops.conv2d(x[i:i + 1].contiguous(), wB, cout, 3, 1, 1, residual=rs[i:i + 1].contiguous(), relu=True, w_layout=BF16X1_3X3, tile=tile)
            assert torch.equal(c, a[i:i + 1]), (tile, i)
        outs[tile] = a
    # every output element is one fixed sequence of MFMAs whatever the form (csrc/conv3x3_bf16x1.hip): the forms agree bit for bit
    assert torch.equal(outs[1], outs[2]) and torch.equal(outs[0], outs[1])


def test_automatic_form_follows_the_documented_rule():
    """tile 0: the form with fewer padded rows (64-row tiles against 96-row tiles), the 64-row form on a tie."""
    from frtm_vos_amd import ops
    for cout, want in ((32, 1), (64, 1), (65, 2), (80, 2), (96, 2), (97, 1), (128, 1), (1, 1)):
        assert (3 * ((cout + 95) // 96) < 2 * ((cout + 63) // 64)) == (want == 2)
        wB, _, _ = ops.pack_weights(torch.ones(cout, 8, 3, 3, device=DEV), bf16x1=True)
        ops.conv2d(torch.ones(1, 8, 4, 4, device=DEV), wB, cout, 3, 1, 1, w_layout=BF16X1_3X3)
        assert _last() == KERNEL[want], (cout, _last())


# ---- 6. argument checks
def _desc(**kw):
    from frtm_vos_amd import _hip as H
    d = dict(B=1, Cin=32, Hin=8, Win=8, Cout=32, ksize=3, stride=1, pad=1, relu=0, out_transposed=0, splitk=0, tile=0, w_layout=BF16X1_3X3, ws_elems=0,
             w_pitch=0)
    d.update(kw)
    return H.ConvDesc(*[d[k] for k, _ in H.ConvDesc._fields_])


@pytest.mark.parametrize('bad', [dict(ksize=1, pad=0), dict(ksize=5, pad=2), dict(stride=2), dict(pad=0), dict(pad=2), dict(out_transposed=1), dict(w_pitch=32),
                                 dict(splitk=2), dict(tile=3), dict(tile=-1), dict(tile=10), dict(misaligned=4), dict(w_layout=BF16X1)])
def test_ineligible_descriptors_are_argument_errors(bad):
    L = _lib()
    x = torch.zeros(1 << 16, device=DEV)
    wB = torch.zeros(1 << 16, device=DEV)
    out = torch.zeros(1 << 16, device=DEV)
    bad = dict(bad)
    off = bad.pop('misaligned', 0)
    d = _desc(**bad)
    before, before1 = _count(), L.frtm_conv_bf16x1_launches()
    rc = L.frtm_conv2d(ctypes.byref(d), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(wB.data_ptr() + off), None, None, None, None,
                       ctypes.c_void_p(out.data_ptr()), None, None)
    assert rc == -1, (bad, rc)
    assert _count() == before and L.frtm_conv_bf16x1_launches() == before1 and _last() == ''
    assert b'frtm_conv2d' in L.frtm_last_error()


def test_ineligible_packs_are_argument_errors():
    L = _lib()
    w = torch.zeros(64 * 40 * 9, device=DEV)
    out = torch.zeros(1 << 16, device=DEV)
    for k, layout, off in ((1, BF16X1_3X3, 0), (3, BF16X1_3X3, 4), (3, BF16X1, 0)):      # (layout 6 still refuses 3x3 kernels)
        rc = L.frtm_conv_pack_weights(ctypes.c_void_p(w.data_ptr()), 64, 32, k, layout, ctypes.c_void_p(out.data_ptr() + off), None, None)
        assert rc == -1 and _last() == '', (k, layout, off)
        assert b'frtm_conv_pack_weights' in L.frtm_last_error()


# ---- 7. refiner
FT = {'layer5': 64, 'layer4': 48, 'layer3': 32, 'layer2': 16}
SIZES = {'layer5': (4, 7), 'layer4': (8, 14), 'layer3': (15, 27), 'layer2': (30, 54)}
IMAGE = (120, 216)


def _refiner_inputs():
    g = torch.Generator().manual_seed(3)
    feats = {L: torch.relu(torch.randn(2, FT[L], *SIZES[L], generator=g)) for L in FT}
    scores = torch.randn(4, 1, 8, 14, generator=g)                           # 2 frames x 2 objects
    return scores, feats


def _rms(t):
    return float(t.double().pow(2).mean().sqrt())


def rule_count(net, samples, frames):
    """3x3 launches per pass that ops.bf16x1_3x3_launch routes: per level the TSE's base conv on the frames, t2, t4 and the four RRB convs on
    the samples, and the head's conv1 on the doubled shallowest map."""
    from frtm_vos_amd import ops
    n = 0
    for L in FT:
        h, w = SIZES[L]
        oc = 64
        for b, cin, cout in ((frames, oc, oc + 1), (samples, oc + 1, oc + 1), (samples, oc + 1, oc)) + ((samples, oc, oc),) * 4:
            n += bool(ops.bf16x1_3x3_launch(b, h, w, cin, cout, net.bf16_min_blocks))
    h, w = SIZES['layer2']
    return n + bool(ops.bf16x1_3x3_launch(samples, 2 * h, 2 * w, 64, 32, net.bf16_min_blocks))


def test_refiner_routes_counts_and_keeps_the_size_of_the_emulated_effect():
    from frtm_vos_amd.model.seg_network import SegNetwork
    torch.set_grad_enabled(False)
    torch.manual_seed(7)
    cpu = SegNetwork(1, 64, dict(FT), use_bn=True).eval()
    scores, feats = _refiner_inputs()
    ref = cpu.forward_torch(scores, feats, IMAGE)
    # the reference definition with the mode's roundings: every 3x3 conv rounds weight and input to bf16 before F.conv2d
    emu = copy.deepcopy(cpu)
    for m in emu.modules():
        if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3):
            m.forward = (lambda mod: lambda t: F.conv2d(t.bfloat16().float(), mod.weight.bfloat16().float(), mod.bias, 1, 1))(m)
    e = _rms(emu.forward_torch(scores, feats, IMAGE) - ref)
    assert e > 0

    net = copy.deepcopy(cpu).to(DEV).eval()
    assert net.precision == 'fp32' and net.bf16_min_blocks is None
    sc, ft = scores.to(DEV), {L: t.to(DEV) for L, t in feats.items()}

    def run():
        a = _count()
        out = net(sc, ft, IMAGE).clone()
        torch.cuda.synchronize()
        return out, _count() - a
    f32, n = run()
    assert n == 0
    net.precision = 'bf16x1'
    out_rule, n = run()
    assert n == rule_count(net, 4, 2), (n, rule_count(net, 4, 2))           # the documented rule on these small maps
    net.bf16_min_blocks = 0
    assert rule_count(net, 4, 2) == 29
    bf, n = run()
    assert n == 29, n                                                        # 7 convs x 4 levels + the head's conv1
    bf2, _ = run()
    assert torch.equal(bf, bf2)
    net.precision = 'fp32'
    back, n = run()
    assert n == 0 and torch.equal(back, f32)                                 # fp32 before and after the switch: bit-identical
    d = _rms(bf.cpu() - f32.cpu())
    print('refiner logits rms %.3e; emulated bf16 effect e = %.3e; HIP bf16x1 - HIP fp32 rms = %.3e; ratio %.3f; HIP fp32 - forward_torch rms %.3e' % (
        _rms(ref), e, d, d / e, _rms(f32.cpu() - ref)))
    assert 0 < d <= 3 * e, (d, e)


# ---- 8. tracker plumbing
def test_tracker_runs_with_a_bf16x1_refiner():
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    torch.set_grad_enabled(False)
    seq = SyntheticSequence('bf16x1r', 6, (128, 160), 2, seed=31)
    seq.preload(DEV)
    labels = {}
    for mode in ('fp32', 'bf16x1'):
        torch.manual_seed(0)
        params = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18', refiner_precision=mode)
        trk = params.get_model().eval()
        assert trk.refiner.precision == mode
        trk.refiner.bf16_min_blocks = 0                                      # the maps of 128x160 frames are below the measured rule's sizes
        a = _count()
        out, _ = trk.run_sequence(seq)
        torch.cuda.synchronize()
        moved = _count() - a
        assert (moved > 0) == (mode == 'bf16x1'), (mode, moved)
        assert len(out) == 6
        for lb in out:
            assert set(int(v) for v in lb.unique().tolist()) <= {0, 1, 2}
        labels[mode] = torch.stack([lb.cpu() for lb in out])
    agree = float((labels['fp32'] == labels['bf16x1']).float().mean())
    print('label agreement of the bf16x1-refiner tracker with the fp32 tracker over 6 frames: %.4f (not gated)' % agree)
