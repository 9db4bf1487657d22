"""The bf16x1_3x3 trunk mode on the GPU: the FRTM_WLAYOUT_BF16X1_3X3_S2 kernel (csrc/conv3x3s2_bf16x1.hip) exactly on bf16-representable data, a
derived error bound on random data, determinism across launches, batches and tile forms, the argument checks; the trunk's routing
(frtm_backbone_set_bf16x1_3x3), the ResNet-18 trunk against a CPU emulation of the same roundings, and a tracker run.

Exact cases: weights in {-1, 0, 1}, activations in {-2 .. 2} (bf16-representable), so every product and every partial sum of up to 9 x 40 of them is a
small integer, exact in fp32 in any order; the epilogue (scale +-{0.5, 1, 2}, quarter-step shift and residual) keeps that.  The output must equal an
fp64 stride-2 convolution BIT FOR BIT.  Buffers are framed: NaN-filled outputs between sentinel bands, NaN-framed inputs and residuals."""
import ctypes
import itertools
import os

import pytest
import torch
from torch.nn import functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = 'cuda'
S1, S2 = 7, 8                 # FRTM_WLAYOUT_BF16X1_3X3, FRTM_WLAYOUT_BF16X1_3X3_S2
TILES = (0, 1, 2)             # frtm_conv_desc.tile: automatic, FRTM_BF16X1_3X3_TILE_64, FRTM_BF16X1_3X3_TILE_96
KERNEL = {1: 'k_conv3x3s2_bf16x1<2>', 2: 'k_conv3x3s2_bf16x1<3>'}
GUARD = 256                   # floats of guard band on each side (a multiple of 4: the framed tensors keep 16-byte alignment)
SENT = 0x7FA5A5A5             # sentinel word (a NaN pattern no kernel produces)


def _lib():
    from frtm_vos_amd import _hip as H
    return H.lib()


def _last():
    return _lib().frtm_conv_last_kernels().decode()


def _counts():
    """(layout-8 launches, layout-7 launches, 1x1 bf16x1 launches)"""
    L = _lib()
    return L.frtm_conv_bf16x1_3x3s2_launches(), L.frtm_conv_bf16x1_3x3_launches(), L.frtm_conv_bf16x1_launches()


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


def _out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def _launch(x, wt, tile=0, scale=None, shift=None, residual=None, relu=False):
    """One framed FRTM_WLAYOUT_BF16X1_3X3_S2 call on CPU operands -> the result on the CPU in fp64; asserts the kernels, the three counters and the
    guard bands."""
    from frtm_vos_amd import ops
    B, cin, h, w = x.shape
    cout = wt.shape[0]
    ho, wo = _out_hw(h, w)
    wB, _, lay = ops.pack_weights(wt.float().to(DEV), bf16x1=True, stride=2)
    assert lay == S2 and _last() == 'k_pack_weights_bf16x1_3x3' and wB.numel() == ops.bf16x1_3x3_elems(cout, cin)
    w7, _, lay7 = ops.pack_weights(wt.float().to(DEV), bf16x1=True)
    assert lay7 == S1 and torch.equal(w7.view(torch.int32), wB.view(torch.int32))          # byte for byte the image of layout 7
    out = Framed(B * cout * ho * wo)
    out.view.fill_(float('nan'))
    c0 = _counts()
    got = ops.conv2d(_nan_framed(x.float()), wB, cout, 3, 2, 1, scale=None if scale is None else scale.float().to(DEV),
                     shift=None if shift is None else shift.float().to(DEV), residual=None if residual is None else _nan_framed(residual.float()),
                     relu=relu, out=out.view.view(B, cout, ho, wo), w_layout=S2, tile=tile)
    assert tuple(got.shape) == (B, cout, ho, wo)
    assert _last() in KERNEL.values() and (tile == 0 or _last() == KERNEL[tile]), _last()
    c1 = _counts()
    assert c1 == (c0[0] + 1, c0[1], c0[2]), (c0, c1)          # its own counter; the layout-7 and 1x1 counters do not move
    torch.cuda.synchronize()
    assert out.intact(), 'output guard band overwritten'
    return out.view.view(B, cout, ho, wo).cpu().double()


def _exact_operands(B, cin, cout, h, w, seed=0):
    g = torch.Generator().manual_seed(seed * 7919 + B * 1009 + cin * 101 + cout * 11 + h + w)
    x = torch.randint(-2, 3, (B, cin, h, w), generator=g).float()
    wt = torch.randint(-1, 2, (cout, cin, 3, 3), generator=g).float()
    ho, wo = _out_hw(h, w)
    sc = (2.0 ** torch.randint(-1, 2, (cout,), generator=g)) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1)
    sh = torch.randint(-8, 9, (cout,), generator=g) / 4.0
    rs = torch.randint(-8, 9, (B, cout, ho, wo), generator=g) / 4.0
    return x, wt, sc, sh, rs


def _ref64(x, wt, sc=None, sh=None, rs=None, relu=False):
    ref = F.conv2d(x.double(), wt.double(), stride=2, padding=1)
    if sc is not None:
        ref = ref * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
    if rs is not None:
        ref = ref + rs.double()
    return torch.relu(ref) if relu else ref


def exact_case(B, cin, cout, h, w, tile, scale=True, res=True, relu=True, seed=0):
    x, wt, sc, sh, rs = _exact_operands(B, cin, cout, h, w, seed)
    got = _launch(x, wt, tile, sc if scale else None, sh if scale else None, rs if res else None, relu)
    label = (B, cin, cout, h, w, tile, scale, res, relu)
    assert not torch.isnan(got).any(), ('unwritten (NaN) outputs: %d' % int(torch.isnan(got).sum()),) + label
    ref = _ref64(x, wt, sc if scale else None, sh if scale else None, rs if res else None, relu)
    bad = got != ref
    assert not bad.any(), ('%d of %d outputs differ, max |err| %g' % (int(bad.sum()), bad.numel(), float((got - ref).abs().max())),) + label


# ---- 1. exact cases
SHAPES = [
    (1, 16, 32, 8, 8),
    (2, 24, 40, 15, 27),       # odd sizes, channel tails, two images
    (1, 16, 72, 20, 70),       # two row tiles, two column tiles, two M tiles
    (3, 32, 96, 9, 66),        # Wo = 33
    (1, 40, 32, 2, 2),
    (1, 16, 32, 1, 1),
]


@pytest.mark.parametrize('tile', TILES)
@pytest.mark.parametrize('B,cin,cout,h,w', SHAPES)
def test_exact_shapes(B, cin, cout, h, w, tile):
    exact_case(B, cin, cout, h, w, tile)


@pytest.mark.parametrize('tile', (1, 2))
@pytest.mark.parametrize('scale,res,relu', list(itertools.product((False, True), repeat=3)))
def test_exact_every_epilogue(scale, res, relu, tile):
    exact_case(2, 24, 40, 15, 27, tile, scale=scale, res=res, relu=relu, seed=1)


@pytest.mark.parametrize('tile', (1, 2))
def test_a_nan_in_image_0_leaves_image_1_finite(tile):
    B, cin, cout, h, w = SHAPES[1]
    x, wt, sc, sh, rs = _exact_operands(B, cin, cout, h, w, seed=2)
    wt = wt.abs() + 1.0                                        # no zero weight: the NaN reaches every window that covers it
    for chan, py, px in ((0, 0, 0), (cin - 1, h - 1, w - 1), (17, 7, 13)):      # corners (the last channel: the tail group of Cin = 24) and the interior
        xv = x.clone()
        xv[0, chan, py, px] = float('nan')
        got = _launch(xv, wt, tile)
        assert bool(torch.isfinite(got[1]).all()), (chan, py, px)
        assert torch.equal(got[1], _ref64(x, wt)[1])
        want = torch.zeros(got.shape[2:], dtype=torch.bool)         # outputs (y, x) with |2 y - py| <= 1 and |2 x - px| <= 1
        for y in range(want.shape[0]):
            for xx in range(want.shape[1]):
                want[y, xx] = abs(2 * y - py) <= 1 and abs(2 * xx - px) <= 1
        assert torch.equal(torch.isnan(got[0]), want.expand_as(got[0])), (chan, py, px)


# ---- 2. error bound on random data
def _bound_case(B, cin, cout, h, w, scale, res, relu, tiles):
    """|out - fp64| <= (2^-7 + 2^-16 + K 2^-22) |scale| (|W| conv |X|) element-wise with K = 9 Cin -- (2u + u^2), u = 2^-8, for the two operand roundings;
    K 2^-22 for K fp32 accumulations with a factor 4 over round-to-nearest for the MFMA's internal sum -- plus the epilogue's own fp32 rounding:
    2^-23 (|scale| |acc| + |value before the residual| + |value after it|), one rounding each for the scaling (or a fused multiply-add), the shift and the
    residual add, with |acc| bounded by |W| conv |X|; a stage that is switched off rounds nothing, so the same expression with scale 1, shift 0 or
    residual 0 bounds it too.  Derived as in tests/test_bf16x1_refiner_gpu.py, not measured."""
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(cin + cout + h)
    x = torch.relu(torch.randn(B, cin, h, w, generator=g)).to(DEV)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(DEV)
    ho, wo = _out_hw(h, w)
    sc = (torch.rand(cout, generator=g) + 0.5).to(DEV)
    sh = (torch.randn(cout, generator=g) * 0.1).to(DEV)
    rs = torch.randn(B, cout, ho, wo, generator=g).to(DEV)
    K = 9 * cin
    s64 = sc.double().view(1, -1, 1, 1) if scale else torch.ones(1, cout, 1, 1, dtype=torch.float64, device=DEV)
    h64 = sh.double().view(1, -1, 1, 1) if scale else torch.zeros(1, cout, 1, 1, dtype=torch.float64, device=DEV)
    r64 = rs.double() if res else torch.zeros(B, cout, ho, wo, dtype=torch.float64, device=DEV)
    mag = F.conv2d(x.double(), wt.double().abs(), stride=2, padding=1)                  # (x >= 0)
    pre = F.conv2d(x.double(), wt.double(), stride=2, padding=1) * s64 + h64
    ref = pre + r64
    if relu:
        ref = torch.relu(ref)
    bound = (2.0 ** -7 + 2.0 ** -16 + K * 2.0 ** -22) * s64.abs() * mag + 2.0 ** -23 * (s64.abs() * mag * (1 + 2.0 ** -6) + pre.abs() + (pre + r64).abs()) * (1 + 2.0 ** -6)
    wB, _, _ = ops.pack_weights(wt, bf16x1=True, stride=2)
    for tile in tiles:
        got = ops.conv2d(x, wB, cout, 3, 2, 1, scale=sc if scale else None, shift=sh if scale else None, residual=rs if res else None, relu=relu,
                         w_layout=S2, tile=tile)
        assert _last() in KERNEL.values() and (tile == 0 or _last() == KERNEL[tile])
        err = (got.double() - ref).abs()
        ratio = float((err / bound.clamp_min(1e-30)).max())
        print('%d->%d %dx%d s2 tile %d (%s) scale %d res %d relu %d: max err %.3e, worst err / bound %.3f' % (
            cin, cout, h, w, tile, _last(), scale, res, relu, float(err.max()), ratio))
        assert bool((err <= bound).all()), (cin, cout, tile, ratio)
        assert float(err.max()) > 1e-5                                      # (the launch really rounded its operands: fp32 kernels sit near 1e-6 here)


@pytest.mark.parametrize('B,cin,cout,h,w', [(2, 64, 128, 30, 54), (1, 128, 256, 24, 40), (2, 24, 40, 15, 27)])
def test_error_within_the_derived_bound(B, cin, cout, h, w):
    _bound_case(B, cin, cout, h, w, True, True, True, TILES)


@pytest.mark.parametrize('scale,res,relu', list(itertools.product((False, True), repeat=3)))
def test_error_bound_every_epilogue(scale, res, relu):
    _bound_case(2, 72, 80, 17, 35, scale, res, relu, (0,))


# ---- 3. determinism: launches, batches, tile forms
def test_bit_identical_across_launches_batches_and_forms():
    from frtm_vos_amd import ops
    B, cin, cout, h, w = 4, 40, 80, 19, 67
    g = torch.Generator().manual_seed(23)
    x = torch.randn(B, cin, h, w, generator=g).to(DEV)
    wt = torch.randn(cout, cin, 3, 3, generator=g).to(DEV)
    ho, wo = _out_hw(h, w)
    rs = torch.randn(B, cout, ho, wo, generator=g).to(DEV)
    wB, _, _ = ops.pack_weights(wt, bf16x1=True, stride=2)
    outs = {}
    for tile in TILES:
        a = ops.conv2d(x, wB, cout, 3, 2, 1, residual=rs, relu=True, w_layout=S2, tile=tile)
        b = ops.conv2d(x, wB, cout, 3, 2, 1, residual=rs, relu=True, w_layout=S2, tile=tile)
        assert torch.equal(a, b), tile
        for i in range(B):                                                   # B = 4 against four B = 1 calls
            c = ops.conv2d(x[i:i + 1].contiguous(), wB, cout, 3, 2, 1, residual=rs[i:i + 1].contiguous(), relu=True, w_layout=S2, tile=tile)
            assert torch.equal(c, a[i:i + 1]), (tile, i)
        outs[tile] = a
    assert torch.equal(outs[1], outs[2]) and torch.equal(outs[0], outs[1])
    assert float((outs[0] - torch.relu(F.conv2d(x, wt, stride=2, padding=1) + rs)).abs().max()) < 0.5      # (a conv, not noise: |out| ~ 19)


def test_automatic_form_follows_the_documented_rule():
    """tile 0: the form with fewer padded rows (64-row tiles against 96-row tiles), the 64-row form on a tie -- the rule of layout 7."""
    from frtm_vos_amd import ops
    for cout, want in ((32, 1), (64, 1), (65, 2), (96, 2), (97, 1), (128, 1)):
        wB, _, _ = ops.pack_weights(torch.ones(cout, 8, 3, 3, device=DEV), bf16x1=True, stride=2)
        ops.conv2d(torch.ones(1, 8, 4, 4, device=DEV), wB, cout, 3, 2, 1, w_layout=S2)
        assert _last() == KERNEL[want], (cout, _last())


# ---- 4. argument checks
def _desc(**kw):
    from frtm_vos_amd import _hip as H
    d = dict(B=1, Cin=32, Hin=8, Win=8, Cout=32, ksize=3, stride=2, pad=1, relu=0, out_transposed=0, splitk=0, tile=0, w_layout=S2, ws_elems=0,
             w_pitch=0)
    d.update(kw)
    return H.ConvDesc(*[d[k] for k, _ in H.ConvDesc._fields_])


@pytest.mark.parametrize('bad', [dict(stride=1), dict(stride=3), dict(ksize=1, pad=0), dict(ksize=5, pad=2), dict(pad=0), dict(pad=2), dict(out_transposed=1),
                                 dict(w_pitch=32), dict(splitk=2), dict(tile=3), dict(tile=-1), dict(tile=10), dict(misaligned=4)])
def test_ineligible_descriptors_are_argument_errors(bad):
    L = _lib()
    x = torch.zeros(1 << 16, device=DEV)
    wB = torch.zeros(1 << 16, device=DEV)
    out = torch.zeros(1 << 16, device=DEV)
    bad = dict(bad)
    off = bad.pop('misaligned', 0)
    d = _desc(**bad)
    before = _counts()
    rc = L.frtm_conv2d(ctypes.byref(d), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(wB.data_ptr() + off), None, None, None, None,
                       ctypes.c_void_p(out.data_ptr()), None, None)
    assert rc == -1, (bad, rc)
    assert _counts() == before and _last() == ''
    assert b'frtm_conv2d' in L.frtm_last_error()


def test_ineligible_packs_are_argument_errors():
    L = _lib()
    w = torch.zeros(64 * 40 * 9, device=DEV)
    out = torch.zeros(1 << 16, device=DEV)
    for k, off in ((1, 0), (3, 4)):
        before = _counts()
        rc = L.frtm_conv_pack_weights(ctypes.c_void_p(w.data_ptr()), 64, 32, k, S2, ctypes.c_void_p(out.data_ptr() + off), None, None)
        assert rc == -1 and _last() == '' and _counts() == before, (k, off)
        assert b'frtm_conv_pack_weights' in L.frtm_last_error()


# ---- 5. trunk routing.  Frames of 96x160 are far below the column counts of a router table measured on 480x854 frames, so the trunks are created under
# FRTM_BF16X1_MIN_COLS=0 (include/frtm_hip.h): every eligible conv is routed.
def _with_min_cols(make, n=0):
    old = os.environ.get('FRTM_BF16X1_MIN_COLS')
    os.environ['FRTM_BF16X1_MIN_COLS'] = str(n)
    try:
        return make()
    finally:
        if old is None:
            del os.environ['FRTM_BF16X1_MIN_COLS']
        else:
            os.environ['FRTM_BF16X1_MIN_COLS'] = old


def conv_census(ext):
    """(indices of the k = 3 stride-1 convs, of the k = 3 stride-2 convs, of the 1x1 stride-1 convs with Cin % 16 == 0) from frtm_backbone_conv_info"""
    from frtm_vos_amd import _hip as H
    info = (ctypes.c_int * 6)()
    s1, s2, one = [], [], []
    for i in range(_lib().frtm_backbone_num_convs(ext._handle)):
        H.call_nostream('frtm_backbone_conv_info', ext._handle, i, info)
        cout, cin, k, s, pad = info[0], info[1], info[2], info[3], info[4]
        if k == 3 and pad == 1 and s == 1:
            s1.append(i)
        elif k == 3 and pad == 1 and s == 2:
            s2.append(i)
        elif k == 1 and s == 1 and cin % 16 == 0:
            one.append(i)
    return s1, s2, one


def _pass(ext, img, **kw):
    a = _counts()
    taps = {k: v.clone() for k, v in ext(img, **kw).items()}
    torch.cuda.synchronize()
    b = _counts()
    return taps, (b[1] - a[1], b[0] - a[0], b[2] - a[2])          # (layout 7, layout 8, 1x1) launches of the pass


_TRUNKS = {}


def _trunk(name):
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    if name not in _TRUNKS:
        ext = _with_min_cols(lambda: ResnetFeatureExtractor(name, seed=0).to(DEV))
        ext.lanes = 1
        img = torch.randint(0, 256, (4, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(11)).to(DEV)
        _TRUNKS[name] = (ext, img, {k: v.clone() for k, v in ext(img).items()})
    return _TRUNKS[name]


@pytest.mark.parametrize('name', ('resnet18', 'resnet50'))
def test_trunk_routing_counts_round_trip_lanes_and_plan(name):
    from frtm_vos_amd import _hip as H
    ext, img, t0 = _trunk(name)
    s1, s2, one = conv_census(ext)
    assert (len(s1), len(s2), len(one)) == {'resnet18': (13, 3, 0), 'resnet50': (13, 3, 33)}[name]
    try:
        ext.lanes = 1
        f32, n = _pass(ext, img)
        assert n == (0, 0, 0) and all(torch.equal(f32[k], t0[k]) for k in t0)
        ext.precision = 'bf16x1'
        b1, n1 = _pass(ext, img)
        assert n1 == (0, 0, len(one)), n1                              # bf16x1 routes the 1x1 convs only
        if name == 'resnet18':
            assert all(torch.equal(b1[k], t0[k]) for k in t0)          # ... of which a BasicBlock trunk has none
        ext.precision = 'bf16x1_3x3'
        assert ext.precision == 'bf16x1_3x3'
        t3, n = _pass(ext, img)
        assert n == (len(s1), len(s2), n1[2]), n                       # one lane of 4 frames: every 3x3 conv, and the 1x1 convs as in bf16x1
        for k in t3:
            assert bool(torch.isfinite(t3[k]).all()), k
            rel = float((t3[k] - t0[k]).abs().max() / t0[k].abs().max())
            print('%s %s: bf16x1_3x3 taps against fp32 taps, max |diff| / max |fp32| = %.3e' % (name, k, rel))
        assert all(not torch.equal(t3[k], t0[k]) for k in ('layer2', 'layer3', 'layer4', 'layer5'))       # (layer1 is the stem: fp32)
        assert torch.equal(t3['layer1'], t0['layer1'])
        # two lanes of 2 frames equal one lane per half, bit for bit; every lane runs every routed conv of its frames
        ext.lanes = 2
        t2, n = _pass(ext, img)
        assert n == (2 * len(s1), 2 * len(s2), 2 * n1[2]), n
        t2s1, n = _pass(ext, img, lane_set=1)
        assert n == (2 * len(s1), 2 * len(s2), 2 * n1[2]), n
        ext.lanes = 1
        ha, n = _pass(ext, img[:2])
        assert n == (len(s1), len(s2), n1[2]), n
        hb, _ = _pass(ext, img[2:])
        for k in t2:
            assert torch.equal(torch.cat([ha[k], hb[k]]), t2[k]), k
            assert torch.equal(t2s1[k], t2[k]), k
            assert torch.equal(t2[k], t3[k]), k                        # ... and the batch of four: independent of the batch size
        # a conv plan keeps its conv on fp32: one launch off the count, for a stride-1 and for a stride-2 conv
        for idx, want in ((s1[2], (len(s1) - 1, len(s2), n1[2])), (s2[1], (len(s1), len(s2) - 1, n1[2]))):
            H.call_nostream('frtm_backbone_set_conv_plan', ext._handle, idx, 1, 0)
            try:
                _, n = _pass(ext, img)
                assert n == want, (idx, n)
            finally:
                H.call_nostream('frtm_backbone_set_conv_plan', ext._handle, idx, 0, 0)
        # bf16x1 is what it was, with a visit to the new mode in between
        ext.precision = 'bf16x1'
        b1b, n = _pass(ext, img)
        assert n == n1 and all(torch.equal(b1b[k], b1[k]) for k in b1)
        # bf16x3 switches the flag off as well
        ext.precision = 'bf16x1_3x3'
        ext.precision = 'bf16x3'
        _, n = _pass(ext, img)
        assert n == (0, 0, 0), n
        # the flag alone (pieces 0 or 3) routes nothing, and a rejected value leaves everything as it was
        H.call_nostream('frtm_backbone_set_bf16x1_3x3', ext._handle, 1)
        _, n = _pass(ext, img)
        assert n == (0, 0, 0), n
        with pytest.raises(RuntimeError):
            H.call_nostream('frtm_backbone_set_bf16x1_3x3', ext._handle, 2)
        ext.precision = 'bf16x1_3x3'
        t3b, n = _pass(ext, img)
        assert n == (len(s1), len(s2), n1[2]) and all(torch.equal(t3b[k], t3[k]) for k in t3)
        # back to fp32: bit-identical to before
        ext.precision = 'fp32'
        f32b, n = _pass(ext, img)
        assert n == (0, 0, 0) and all(torch.equal(f32b[k], t0[k]) for k in t0)
    finally:
        ext.precision = 'fp32'
        ext.lanes = 1


def conv_inputs(ext, H, W):
    """[(idx, (Cout, Cin, k, stride, pad), (Hin, Win))] in forward order: the stem at the frame; per block conv1 [conv2] [conv3] [downsample], the
    first block of stages 1..3 on the previous stage's map, which only its strided conv (the 3x3 of a bottleneck, conv1 of a BasicBlock) and its
    downsample leave."""
    from frtm_vos_amd import _hip as H_
    info, shapes = (ctypes.c_int * 6)(), []
    for i in range(_lib().frtm_backbone_num_convs(ext._handle)):
        H_.call_nostream('frtm_backbone_conv_info', ext._handle, i, info)
        shapes.append(tuple(info[:5]))
    bott = hasattr(ext.resnet.layer1[0], 'conv3')
    half = lambda hw: ((hw[0] + 1) // 2, (hw[1] + 1) // 2)          # noqa: E731
    out, i, cur = [(0, shapes[0], (H, W))], 1, half(half((H, W)))
    for s in range(4):
        for b, blk in enumerate(getattr(ext.resnet, 'layer%d' % (s + 1))):
            own = half(cur) if (s > 0 and b == 0) else cur
            for j in range(3 if bott else 2):
                out.append((i, shapes[i], cur if j <= (1 if bott else 0) else own))
                i += 1
            if hasattr(blk, 'downsample'):
                out.append((i, shapes[i], cur))
                i += 1
            cur = own
    assert i == len(shapes)
    return out


@pytest.mark.parametrize('name', ('resnet18', 'resnet50'))
def test_the_pass_takes_the_routes_the_query_reports(name):
    """frtm_backbone_conv_route decides from the modes alone (csrc/trunk_route.h: wanted_images); the pass decides from the images the convs really hold.
    Per mode the launch counters of a pass and its four FLOP ledgers must be what the query says for every conv at its own input size."""
    ext, img, _ = _trunk(name)
    B = img.shape[0]
    convs = conv_inputs(ext, 96, 160)
    out3 = (ctypes.c_int * 3)()
    try:
        ext.lanes = 1
        seen = set()
        for mode in ('fp32', 'bf16x1', 'bf16x1_3x3'):
            ext.precision = mode
            want_n, want_flops = {S1: 0, S2: 0, 6: 0}, [0.0, 0.0, 0.0, 0.0]
            for idx, (cout, cin, k, s, pad), (h, w) in convs:
                assert _lib().frtm_backbone_conv_route(ext._handle, idx, B, h, w, out3) == 0
                lay, _, slot = tuple(out3)
                if lay in want_n:
                    want_n[lay] += 1
                seen.add(lay)
                ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
                want_flops[slot] += 2.0 * cout * B * ho * wo * cin * k * k
            _, n = _pass(ext, img)
            assert n == (want_n[S1], want_n[S2], want_n[6]), (mode, n, want_n)
            assert list(ext.last_flops_form) == want_flops, (mode, ext.last_flops_form, want_flops)
            assert ext.last_flops == sum(want_flops) and ext.last_conv_launches == len(convs)
        assert {0, 1, S1, S2} <= seen and (name == 'resnet18' or 6 in seen), seen          # (the query was asked about routes of every kind)
    finally:
        ext.precision = 'fp32'


def test_reupload_packs_the_3x3_images_again():
    """frtm_backbone_set_conv after the flag is on packs the bf16 images from the new weights (here: the same ones, so the taps are bit-identical)."""
    ext, img, _ = _trunk('resnet18')
    try:
        ext.precision = 'bf16x1_3x3'
        a, n = _pass(ext, img)
        ext.upload()
        b, m = _pass(ext, img)
        assert n == m == (13, 3, 0) and all(torch.equal(a[k], b[k]) for k in a)
        w = ext.resnet.layer2[0].conv1.weight                     # the stride-2 conv that opens layer2
        old = w.data.clone()
        w.data.mul_(2.0)
        ext.upload()
        c, _ = _pass(ext, img)
        assert not torch.equal(c['layer3'], a['layer3'])
        w.data.copy_(old)
        ext.upload()
        d, _ = _pass(ext, img)
        assert all(torch.equal(a[k], d[k]) for k in a)
    finally:
        ext.precision = 'fp32'


# (Cin, Cout, stride) -> fewest columns per launch from which trunk_route.h's kTrunkRules routes the shape (profiles/bf16x1_trunk3x3_time.txt)
DEFAULT_RULES_3X3 = {(64, 64, 1): 25680, (128, 128, 1): 6420, (256, 256, 1): 12960, (512, 512, 1): 3240, (128, 128, 2): 6420, (256, 256, 2): 12960,
                     (512, 512, 2): 3240, (64, 128, 2): 6420, (128, 256, 2): 1620, (256, 512, 2): 3240}


def default_table_count_3x3(name, cols):
    """(layout 7, layout 8) launches per pass in one lane under DEFAULT_RULES_3X3; cols[s] = columns (frames x pixels) of stage s's OUTPUT map.  A
    stage's 3x3 convs all write its own map (the stride-2 conv that opens stage s included)."""
    blocks = {'resnet18': (2, 2, 2, 2), 'resnet50': (3, 4, 6, 3)}[name]
    basic = name == 'resnet18'
    n7 = n8 = 0
    for s in range(4):
        c = 64 << s
        per_block = 2 if basic else 1                                       # 3x3 convs c -> c per block
        n_s1 = blocks[s] * per_block - (1 if s > 0 else 0)                  # ... but the opening conv of stages 1..3 has stride 2
        if DEFAULT_RULES_3X3.get((c, c, 1), 1 << 62) <= cols[s]:
            n7 += n_s1
        if s > 0 and DEFAULT_RULES_3X3.get((c // 2 if basic else c, c, 2), 1 << 62) <= cols[s]:
            n8 += 1
    return n7, n8


@pytest.mark.parametrize('name', ('resnet18', 'resnet50'))
def test_default_router_table_routes_nothing_on_small_frames(name, monkeypatch):
    """Without the knob the table holds column counts measured on 480x854 frames: two frames of 96x160 (at most 1920 columns per launch) route what
    the table implies at that size -- nothing, unless a rule reaches that far down."""
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    monkeypatch.delenv('FRTM_BF16X1_MIN_COLS', raising=False)
    ext = ResnetFeatureExtractor(name, seed=0).to(DEV)
    small = torch.randint(0, 256, (2, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(13)).to(DEV)
    f32, _ = _pass(ext, small)
    ext.precision = 'bf16x1'
    b1, n1 = _pass(ext, small)
    ext.precision = 'bf16x1_3x3'
    want = default_table_count_3x3(name, {0: 2 * 24 * 40, 1: 2 * 12 * 20, 2: 2 * 6 * 10, 3: 2 * 3 * 5})
    taps, n = _pass(ext, small)
    assert n == want + (n1[2],), (n, want)
    if want == (0, 0):
        assert all(torch.equal(taps[k], b1[k]) for k in b1)


def test_default_router_table_at_full_size():
    """One 480x854 frame through ResNet-18 without the knob: layer1's four convs (25680 columns), layer2's three stride-1 convs and its opener (6420),
    layer3's opener (1620); nothing of layer3's stride-1 convs (routed from 12960 columns on) or of layer4 (from 3240)."""
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    old = os.environ.pop('FRTM_BF16X1_MIN_COLS', None)
    try:
        ext = ResnetFeatureExtractor('resnet18', seed=0).to(DEV)
    finally:
        if old is not None:
            os.environ['FRTM_BF16X1_MIN_COLS'] = old
    big = torch.randint(0, 256, (1, 3, 480, 854), dtype=torch.uint8, generator=torch.Generator().manual_seed(12)).to(DEV)
    ext.precision = 'bf16x1_3x3'
    want = default_table_count_3x3('resnet18', {0: 120 * 214, 1: 60 * 107, 2: 30 * 54, 3: 15 * 27})
    assert want == (4 + 3, 2)
    taps, n = _pass(ext, big)
    assert n == want + (0,), n
    assert all(bool(torch.isfinite(v).all()) for v in taps.values())


def test_graph_recaptured_on_mode_switch():
    ext, img, t0 = _trunk('resnet18')
    ext.lanes = 1
    ext.precision = 'bf16x1_3x3'
    eager, _ = _pass(ext, img)
    ext.precision = 'fp32'
    ext.reuse_outputs, ext.use_graph = True, True
    try:
        for _ in range(3):
            f32 = ext(img)
        f32 = {k: v.clone() for k, v in f32.items()}
        assert any(e['graph'] is not None for e in ext._out_cache.values())
        ext.precision = 'bf16x1_3x3'
        assert not ext._out_cache
        a = _counts()
        for _ in range(3):
            out = ext(img)
        torch.cuda.synchronize()
        assert any(e['graph'] is not None for e in ext._out_cache.values())
        assert _counts()[0] > a[0] and _counts()[1] > a[1]
        for k in eager:
            assert torch.equal(out[k], eager[k]), k
            assert torch.equal(f32[k], t0[k]), k
        assert any(not torch.equal(out[k], f32[k]) for k in eager)
        # ... and from bf16x1 to bf16x1_3x3: the pieces stay 1, only the flag changes, and that alone re-captures
        ext.precision = 'bf16x1'
        for _ in range(3):
            out = ext(img)
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], t0[k]) for k in t0)             # (ResNet-18: bf16x1 is fp32)
        ext.precision = 'bf16x1_3x3'
        for _ in range(3):
            out = ext(img)
        torch.cuda.synchronize()
        assert all(torch.equal(out[k], eager[k]) for k in eager)
    finally:
        ext.reuse_outputs, ext.use_graph = False, False
        ext.precision = 'fp32'
        ext._out_cache.clear()


# ---- 6. the ResNet-18 trunk against an emulation of its roundings
def _bf16(t):
    return t.float().bfloat16().double()


def _emulate_resnet18(ext, img_u8, round_3x3):
    """fp64 forward of the BasicBlock trunk on the CPU from the extractor's own parameters (BatchNorm folded as upload() folds it); round_3x3: both
    operands of every 3x3 conv rounded to bf16 (to nearest even), as the bf16x1_3x3 mode does."""
    r = ext.resnet

    def fold(bn):
        scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).float()
        shift = (bn.bias - bn.running_mean * scale).float()
        return scale.double().cpu().view(1, -1, 1, 1), shift.double().cpu().view(1, -1, 1, 1)

    def conv_bn(x, cv, bn, stride, pad):
        w = cv.weight.data.double().cpu()
        if round_3x3 and w.shape[-1] == 3:
            x, w = _bf16(x), _bf16(w)
        s, b = fold(bn)
        return F.conv2d(x, w, stride=stride, padding=pad) * s + b
    x = img_u8.double().cpu() * ext.norm_weight.double().cpu() + ext.norm_bias.double().cpu()
    x = torch.relu(conv_bn(x, r.conv1, r.bn1, 2, 3))
    taps = {'layer1': x}
    x = F.max_pool2d(x, 3, 2, 1)
    for li in range(1, 5):
        for blk in getattr(r, 'layer%d' % li):
            idn = x
            if hasattr(blk, 'downsample'):
                idn = conv_bn(x, blk.downsample[0], blk.downsample[1], blk.downsample[0].stride, 0)
            y = torch.relu(conv_bn(x, blk.conv1, blk.bn1, blk.conv1.stride, 1))
            x = torch.relu(conv_bn(y, blk.conv2, blk.bn2, 1, 1) + idn)
        taps['layer%d' % (li + 1)] = x
    return taps


EMULATION_MARGIN = 1.252          # 1.25 x 1.0015, the largest ratio measured on an MI355X (layer2 .. layer5: 1.000, 0.984, 1.001, 0.993)


def test_resnet18_trunk_against_the_emulated_roundings():
    """Per tap: max |HIP bf16x1_3x3 - plain fp64| <= m x max |emulation - plain fp64|, the emulation being the same fp64 forward with both operands of
    every 3x3 conv rounded to bf16.  The margin m exists because the HIP trunk rounds fp32 activations where the emulation rounds fp64 ones, so single
    roundings flip; a wrong weight image or epilogue misses by orders of magnitude.  m = the ratio measured on the GPU x 1.25, never above 2.
    Measured on an MI355X: ratios 1.000 (layer2), 0.984 (layer3), 1.001 (layer4: 8.3731e-03 / 8.3611e-03), 0.993 (layer5), so m = 1.25 x 1.0015 = 1.252
    (EMULATION_MARGIN; recorded in profiles/bf16x1_trunk3x3_time.txt).  The fp32 trunk must sit orders of magnitude below the emulation's
    deviation (the gate is about the roundings, not about fp32 noise)."""
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    ext = _with_min_cols(lambda: ResnetFeatureExtractor('resnet18', seed=4).to(DEV))
    ext.lanes = 1
    img = torch.randint(0, 256, (2, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    plain, emu = _emulate_resnet18(ext, img, False), _emulate_resnet18(ext, img, True)
    f32, n = _pass(ext, img.to(DEV))
    assert n == (0, 0, 0)
    ext.precision = 'bf16x1_3x3'
    hip, n = _pass(ext, img.to(DEV))
    assert n == (13, 3, 0), n
    for k in ('layer2', 'layer3', 'layer4', 'layer5'):
        d_hip = float((hip[k].double().cpu() - plain[k]).abs().max())
        d_emu = float((emu[k] - plain[k]).abs().max())
        d_f32 = float((f32[k].double().cpu() - plain[k]).abs().max())
        d_he = float((hip[k].double().cpu() - emu[k]).abs().max())
        print('resnet18 %s: max|HIP - plain| %.4e, max|emulation - plain| %.4e, ratio %.3f (m = %.3f); max|HIP - emulation| %.3e; fp32 trunk - plain %.3e; max|plain| %.3e' % (
            k, d_hip, d_emu, d_hip / d_emu, EMULATION_MARGIN, d_he, d_f32, float(plain[k].abs().max())))
        assert d_emu > 100 * d_f32, k
        assert d_hip <= EMULATION_MARGIN * d_emu, (k, d_hip, d_emu)
    assert torch.equal(hip['layer1'], f32['layer1'])          # the stem stays fp32


def test_trunk_vs_oracle_is_printed_not_gated():
    """Taps of the bf16x1_3x3 trunk against the CPU oracle, per tap, next to the fp32 trunk's: printed (and recorded at full size in
    profiles/bf16x1_trunk3x3_time.txt).  No numeric gate: the figure cannot be derived, and it must not be set from the code under test."""
    from oracle import cpu_ref as O
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    for name in ('resnet18', 'resnet50'):
        P = O.resnet_random_params(name, seed=3)
        img = torch.randint(0, 256, (4, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
        ref = O.resnet_forward(name, P, img)
        ext = _with_min_cols(lambda: ResnetFeatureExtractor(name, weights=P).to(DEV))
        ext.lanes = 1
        out = {}
        for mode in ('fp32', 'bf16x1', 'bf16x1_3x3'):
            ext.precision = mode
            out[mode], n = _pass(ext, img.to(DEV))
            assert (n[0], n[1]) == ((13, 3) if mode == 'bf16x1_3x3' else (0, 0)), (mode, n)
        for k in sorted(ref):
            e = [float((out[m][k].double().cpu() - ref[k].double()).abs().max() / (ref[k].double().abs().max() + 1e-30)) for m in ('fp32', 'bf16x1', 'bf16x1_3x3')]
            print('%s B=4 %s: rel err against the oracle fp32 %.3e bf16x1 %.3e bf16x1_3x3 %.3e' % (name, k, e[0], e[1], e[2]))
            assert bool(torch.isfinite(out['bf16x1_3x3'][k]).all()), k


# ---- 7. tracker plumbing
def test_tracker_runs_with_a_bf16x1_3x3_resnet18_trunk():
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    torch.set_grad_enabled(False)
    seq = SyntheticSequence('bf16x1_3x3', 6, (128, 160), 2, seed=31)
    seq.preload(DEV)
    labels = {}
    for mode in ('fp32', 'bf16x1_3x3'):
        torch.manual_seed(0)
        params = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18', trunk_precision=mode)
        trk = _with_min_cols(lambda: params.get_model().eval())          # every eligible conv of the trunk is routed
        assert trk.feature_extractor.precision == mode
        a = _counts()
        out, _ = trk.run_sequence(seq)
        torch.cuda.synchronize()
        b = _counts()
        moved = (b[0] - a[0], b[1] - a[1])
        assert (moved[0] > 0 and moved[1] > 0) if mode == 'bf16x1_3x3' else moved == (0, 0), (mode, moved)
        assert b[2] == a[2]                                              # ResNet-18 has no 1x1 conv to route
        assert len(out) == 6
        for lb in out:
            assert set(int(v) for v in lb.unique().tolist()) <= {0, 1, 2}
        labels[mode] = torch.stack([lb.cpu() for lb in out])
    agree = float((labels['fp32'] == labels['bf16x1_3x3']).float().mean())
    print('label agreement of the bf16x1_3x3 ResNet-18 tracker with the fp32 tracker over 6 frames: %.4f (not gated)' % agree)
