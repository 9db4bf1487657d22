"""The bf16x1 trunk mode on the GPU: the FRTM_WLAYOUT_BF16X1 1x1 kernel (csrc/conv_bf16x1.hip) exactly on bf16-representable data, its rounding
(to nearest even, on both operands), a derived error bound on realistic data, determinism across launches, grids and tile forms, the argument checks,
the trunk's routing, graph re-capture and a tracker run with a bf16x1 trunk.

Exact cases: operands are integers in [-15, 15] (bf16 holds 8 significant bits), so every product and every partial sum of up to 256 of them is an
integer below 2^24 and exact in fp32 in any order; the epilogue (scale +-{0.5, 1, 2}, quarter-step shift and residual) keeps that.  The output must
equal an fp64 convolution BIT FOR BIT.  Buffers are framed: NaN-filled outputs between sentinel bands, NaN-framed inputs and residuals.

The mode is defined by its arithmetic (sections 1-3), not by parity with the oracle: the trunk and tracker tests print how far the taps and the
labels move and gate on plumbing only."""
import ctypes
import itertools
import os

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = 'cuda'
BF16X1 = 6
TILES = (0, 1, 2)             # frtm_conv_desc.tile: automatic, FRTM_BF16X1_TILE_128x64, FRTM_BF16X1_TILE_64x64
KERNEL = {1: 'k_conv1x1_bf16x1<128,64,64>', 2: 'k_conv1x1_bf16x1<64,64,64>'}
GUARD = 256                   # floats of guard band on each side (a multiple of 4: the framed tensors keep 16-byte alignment)
SENT = 0x7FA5A5A5             # sentinel word (a NaN pattern no kernel produces)


def _lib():
    from frtm_vos_amd import _hip as H
    return H.lib()


def _last():
    return _lib().frtm_conv_last_kernels().decode()


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


def bf_case(B, cin, cout, h, w, tile, scale=False, res=False, relu=False, seed=0):
    """One FRTM_WLAYOUT_BF16X1 call on framed buffers; asserts the kernels, the guard bands and the exact result."""
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(seed * 7919 + B * 1009 + cin * 101 + cout * 11 + h + w)
    x, wt = _ints(g, (B, cin, h, w)), _ints(g, (cout, cin, 1, 1))
    sc = (2.0 ** torch.randint(-1, 2, (cout,), generator=g)) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1)
    sh = torch.randint(-8, 9, (cout,), generator=g) / 4.0
    rs = torch.randint(-8, 9, (B, cout, h, w), generator=g) / 4.0
    wB, _, lay = ops.pack_weights(wt.to(DEV), bf16x1=True)
    assert lay == BF16X1 and _last() == 'k_pack_weights_bf16x1' and wB.numel() == ops.bf16x1_elems(cout, cin)
    out = Framed(B * cout * h * w)
    out.view.fill_(float('nan'))
    n0 = _lib().frtm_conv_bf16x1_launches()
    ops.conv2d(_nan_framed(x), wB, cout, 1, 1, 0, scale=sc.float().to(DEV) if scale else None, shift=sh.float().to(DEV) if scale else None,
               residual=_nan_framed(rs.float()) if res else None, relu=relu, out=out.view.view(B, cout, h, w), w_layout=BF16X1, tile=tile)
    assert _last() in KERNEL.values() and (tile == 0 or _last() == KERNEL[tile]), _last()
    assert _lib().frtm_conv_bf16x1_launches() == n0 + 1
    torch.cuda.synchronize()
    label = (B, cin, cout, h, w, tile, scale, res, relu)
    assert out.intact(), ('output guard band overwritten',) + label
    got = out.view.view(B, cout, h, w).cpu().double()
    assert not torch.isnan(got).any(), ('unwritten (NaN) outputs: %d' % int(torch.isnan(got).sum()),) + label
    ref = torch.einsum('mk,bkp->bmp', wt.double().view(cout, cin), x.double().view(B, cin, -1)).view(B, cout, h, w)
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
    (2, 48, 65, 6, 10),        # Cout tail, K = 48: three of a chunk's four k-steps, one pixel tile across both images
    (1, 16, 130, 11, 13),      # B = 1, one k-step (a quarter chunk), two / three Cout tiles, 143 pixels (odd, ragged tile)
    (8, 64, 256, 15, 27),      # B = 8 on the layer4 map size (405 pixels: tiles straddle images), Cout multiple of the tile
    (3, 32, 33, 7, 9),
    (8, 256, 96, 4, 5),        # 256-deep K (four chunks: both register sets and LDS stages twice), 20-pixel images: a tile spans seven images
])
def test_exact_shapes(B, cin, cout, h, w, tile):
    bf_case(B, cin, cout, h, w, tile, scale=True, res=True, relu=True)


@pytest.mark.parametrize('tile', (1, 2))
@pytest.mark.parametrize('scale,res,relu', list(itertools.product((False, True), repeat=3)))
def test_exact_every_epilogue(scale, res, relu, tile):
    bf_case(2, 80, 72, 9, 7, tile, scale=scale, res=res, relu=relu, seed=1)


def test_exact_data_is_exact_in_fp32_at_k_256():
    """The claim the exact cases rest on, on the CPU: with K = 256 the fp32 sum (in torch's order) equals the fp64 sum."""
    g = torch.Generator().manual_seed(5)
    x, wt = _ints(g, (2, 256, 40)), _ints(g, (96, 256))
    assert torch.equal(torch.einsum('mk,bkp->bmp', wt, x).double(), torch.einsum('mk,bkp->bmp', wt.double(), x.double()))
    assert torch.equal(x.bfloat16().float(), x) and torch.equal(wt.bfloat16().float(), wt)       # bf16-representable


# ---- 2. rounding: to nearest even, on both operands
RNE_VALUES = (1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -7 - 2.0 ** -20, 1.5 + 2.0 ** -9)
RNE_ROUNDED = (1.0, 1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 1 + 2.0 ** -7, 1.5)      # ties (entries 1-3) go to the even neighbour


def _rne_operands(g, B, cin, cout, h, w):
    vals = torch.tensor(RNE_VALUES, dtype=torch.float64)

    def draw(shape):
        v = vals[torch.randint(0, len(RNE_VALUES), shape, generator=g)]
        return (v * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()
    x, wt = draw((B, cin, h, w)), draw((cout, cin))
    period = max(1, (cin + 15) // 16)                                  # at most 16 non-zero weights per output channel
    m, k = torch.meshgrid(torch.arange(cout), torch.arange(cin), indexing='ij')
    return x, wt * (((m + k) % period) == 0).float()


def _truncated(t):
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


@pytest.mark.parametrize('tile', (1, 2))
def test_operands_are_rounded_to_nearest_even(tile):
    from frtm_vos_amd import ops
    B, cin, cout, h, w = 2, 80, 72, 9, 7
    g = torch.Generator().manual_seed(17)
    x, wt = _rne_operands(g, B, cin, cout, h, w)
    assert int((wt != 0).sum(1).max()) <= 16
    # torch rounds these values as the kernel must: the ties to the even neighbour
    assert torch.equal(torch.tensor(RNE_VALUES, dtype=torch.float32).bfloat16().double(), torch.tensor(RNE_ROUNDED, dtype=torch.float64))

    def prod(wv, xv):
        return torch.einsum('mk,bkp->bmp', wv.double(), xv.double().view(B, cin, -1)).view(B, cout, h, w)
    ref = prod(wt.bfloat16(), x.bfloat16())
    assert torch.equal(prod(wt.bfloat16(), x.bfloat16()).float().double(), ref)          # sums of 16 such products are exact in fp32
    # the data discriminates: truncation of either operand, or no rounding at all, gives another result somewhere
    assert not torch.equal(prod(_truncated(wt), _truncated(x)), ref)
    assert not torch.equal(prod(_truncated(wt), x.bfloat16()), ref) and not torch.equal(prod(wt.bfloat16(), _truncated(x)), ref)
    assert not torch.equal(prod(wt, x), ref)
    wB, _, _ = ops.pack_weights(wt.view(cout, cin, 1, 1).to(DEV), bf16x1=True)
    out = Framed(B * cout * h * w)
    out.view.fill_(float('nan'))
    ops.conv2d(_nan_framed(x), wB, cout, 1, 1, 0, out=out.view.view(B, cout, h, w), w_layout=BF16X1, tile=tile)
    assert _last() == KERNEL[tile]
    torch.cuda.synchronize()
    got = out.view.view(B, cout, h, w).cpu().double()
    assert out.intact() and not torch.isnan(got).any()
    bad = got != ref
    assert not bad.any(), '%d of %d outputs differ from the round-to-nearest-even product, max |err| %g' % (
        int(bad.sum()), bad.numel(), float((got - ref).abs().max()))


# ---- 3. error bound on realistic data
@pytest.mark.parametrize('B,cin,cout,h,w', [(2, 256, 1024, 30, 54), (2, 1024, 256, 30, 54), (2, 64, 256, 24, 40)])
def test_error_within_the_derived_bound(B, cin, cout, h, w):
    """|out - fp64| <= (2^-7 + 2^-16 + K 2^-22) (|W|.|X|) element-wise: (2u + u^2), u = 2^-8, for the two operand roundings; K 2^-22 for K fp32
    accumulations with a factor 4 over round-to-nearest for the MFMA's internal sum.  Derived, not measured.  The kernel's max error must also
    exceed the fp32 kernel's on the same data: the launch really took the bf16 form."""
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.relu(torch.randn(B, cin, h, w, generator=g)).to(DEV)
    wt = (torch.randn(cout, cin, 1, 1, generator=g) / cin ** 0.5).to(DEV)
    X, W = x.double().reshape(B, cin, -1), wt.double().reshape(cout, cin)
    ref = torch.matmul(W, X)
    bound = (2.0 ** -7 + 2.0 ** -16 + cin * 2.0 ** -22) * torch.matmul(W.abs(), X.abs())
    wT, kt, lay = ops.pack_weights(wt)
    e32 = (ops.conv2d(x, wT, cout, 1, 1, 0, ktab=kt, w_layout=lay).double().reshape(B, cout, -1) - ref).abs()
    wB, _, _ = ops.pack_weights(wt, bf16x1=True)
    for tile in TILES:
        got = ops.conv2d(x, wB, cout, 1, 1, 0, w_layout=BF16X1, tile=tile)
        assert _last() in KERNEL.values() and (tile == 0 or _last() == KERNEL[tile])
        err = (got.double().reshape(B, cout, -1) - ref).abs()
        print('%d->%d tile %d (%s): max err bf16x1 %.3e (fp32 kernel %.3e), worst err / bound %.3f' % (
            cin, cout, tile, _last(), float(err.max()), float(e32.max()), float((err / bound.clamp_min(1e-30)).max())))
        assert bool((err <= bound).all()), (cin, cout, tile, float((err / bound.clamp_min(1e-30)).max()))
        assert float(err.max()) > float(e32.max()), (cin, cout, tile, float(err.max()), float(e32.max()))


# ---- 4. determinism: launches, grids, tile forms
def test_bit_identical_across_launches_sub_batches_and_forms():
    from frtm_vos_amd import ops
    B, cin, cout, h, w = 3, 80, 200, 13, 17
    g = torch.Generator().manual_seed(23)
    x = torch.randn(B, cin, h, w, generator=g).to(DEV)
    wt = torch.randn(cout, cin, 1, 1, generator=g).to(DEV)
    rs = torch.randn(B, cout, h, w, generator=g).to(DEV)
    wB, _, _ = ops.pack_weights(wt, bf16x1=True)
    outs = {}
    for tile in TILES:
        a = ops.conv2d(x, wB, cout, 1, 1, 0, residual=rs, relu=True, w_layout=BF16X1, tile=tile)
        b = ops.conv2d(x, wB, cout, 1, 1, 0, residual=rs, relu=True, w_layout=BF16X1, tile=tile)
        assert torch.equal(a, b), tile
        # a sub-batch computes the same columns bit for bit (other grid size, other tile boundaries)
        c = ops.conv2d(x[1:2].contiguous(), wB, cout, 1, 1, 0, residual=rs[1:2].contiguous(), relu=True, w_layout=BF16X1, tile=tile)
        assert torch.equal(c, a[1:2]), tile
        outs[tile] = a
    # every output element is one fixed sequence of MFMAs whatever the form (csrc/conv_bf16x1.hip): the forms agree bit for bit
    assert torch.equal(outs[1], outs[2]) and torch.equal(outs[0], outs[1])


def test_automatic_form_follows_the_documented_rule():
    """tile 0: FRTM_BF16X1_TILE_128x64 for Cin >= 1024 when that form has at least one tile per CU, else FRTM_BF16X1_TILE_64x64 -- on both sides of
    the column threshold, and below the K threshold; the two choices agree bit for bit."""
    from frtm_vos_amd import ops
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cout = 256                                                            # two 128-row tiles: the large form has 2 ceil(columns / 64) tiles
    cols = 64 * ((cus + 1) // 2)                                          # fewest columns (a multiple of 64) that give it >= cus tiles
    g = torch.Generator().manual_seed(29)
    for cin, n, want in ((1024, cols, 1), (1024, cols - 64, 2), (960, cols, 2)):
        x = torch.randn(1, cin, 1, n, generator=g).to(DEV)
        wB, _, _ = ops.pack_weights(torch.randn(cout, cin, 1, 1, generator=g).to(DEV), bf16x1=True)
        a = ops.conv2d(x, wB, cout, 1, 1, 0, w_layout=BF16X1)
        assert _last() == KERNEL[want], (cin, n, _last())
        b = ops.conv2d(x, wB, cout, 1, 1, 0, w_layout=BF16X1, tile=3 - want)
        assert _last() == KERNEL[3 - want] and torch.equal(a, b), (cin, n)


# ---- 5. argument checks
def _desc(**kw):
    from frtm_vos_amd import _hip as H
    d = dict(B=1, Cin=32, Hin=8, Win=8, Cout=32, ksize=1, stride=1, pad=0, relu=0, out_transposed=0, splitk=0, tile=0, w_layout=BF16X1, ws_elems=0,
             w_pitch=0)
    d.update(kw)
    return H.ConvDesc(*[d[k] for k, _ in H.ConvDesc._fields_])


@pytest.mark.parametrize('bad', [dict(ksize=3, pad=1), dict(stride=2), dict(pad=1, ksize=1), dict(out_transposed=1), dict(w_pitch=32), dict(Cin=40),
                                 dict(tile=3), dict(tile=-1), dict(tile=23), dict(splitk=2), dict(misaligned=4)])
def test_ineligible_descriptors_are_argument_errors(bad):
    L = _lib()
    x = torch.zeros(1 << 16, device=DEV)
    wB = torch.zeros(1 << 16, device=DEV)
    out = torch.zeros(1 << 16, device=DEV)
    bad = dict(bad)
    off = bad.pop('misaligned', 0)
    d = _desc(**bad)
    before, before3 = L.frtm_conv_bf16x1_launches(), L.frtm_conv_bf16x3_launches()
    rc = L.frtm_conv2d(ctypes.byref(d), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(wB.data_ptr() + off), None, None, None, None,
                       ctypes.c_void_p(out.data_ptr()), None, None)
    assert rc == -1, (bad, rc)
    assert L.frtm_conv_bf16x1_launches() == before and L.frtm_conv_bf16x3_launches() == before3 and _last() == ''
    assert b'frtm_conv2d' in L.frtm_last_error()


def test_ineligible_packs_are_argument_errors():
    L = _lib()
    w = torch.zeros(64 * 40 * 9, device=DEV)
    out = torch.zeros(1 << 16, device=DEV)
    for cin, k, off in ((40, 1, 0), (32, 3, 0), (32, 1, 4)):
        rc = L.frtm_conv_pack_weights(ctypes.c_void_p(w.data_ptr()), 64, cin, k, BF16X1, ctypes.c_void_p(out.data_ptr() + off), None, None)
        assert rc == -1 and _last() == '', (cin, k, off)
        assert b'frtm_conv_pack_weights' in L.frtm_last_error()


def test_a_valid_launch_counts_once_and_not_as_bf16x3():
    from frtm_vos_amd import ops
    L = _lib()
    wB, _, _ = ops.pack_weights(torch.ones(32, 32, 1, 1, device=DEV), bf16x1=True)
    a1, a3 = L.frtm_conv_bf16x1_launches(), L.frtm_conv_bf16x3_launches()
    y = ops.conv2d(torch.ones(1, 32, 8, 8, device=DEV), wB, 32, 1, 1, 0, w_layout=BF16X1)
    assert L.frtm_conv_bf16x1_launches() == a1 + 1 and L.frtm_conv_bf16x3_launches() == a3
    assert bool((y == 32).all())


# ---- 6. trunk routing.  Frames of 96x160 are far below the column counts of the router's measured table (480x854 frames), so the trunk is created
# under FRTM_BF16X1_MIN_COLS (include/frtm_hip.h: frtm_backbone_set_bf16_pieces): every eligible conv is routed from MIN_COLS columns per launch on.
MIN_COLS = 480
HW = {0: 24 * 40, 1: 12 * 20, 2: 6 * 10, 3: 3 * 5}          # pixels per frame of layer1..layer4's maps for 96x160 frames


def _with_min_cols(make, n=MIN_COLS):
    old = os.environ.get('FRTM_BF16X1_MIN_COLS')
    os.environ['FRTM_BF16X1_MIN_COLS'] = str(n)
    try:
        return make()
    finally:
        if old is None:
            del os.environ['FRTM_BF16X1_MIN_COLS']
        else:
            os.environ['FRTM_BF16X1_MIN_COLS'] = old


def routed_convs(ext, lane_frames, min_cols=MIN_COLS):
    """Indices of the convs a bf16x1 trunk created under FRTM_BF16X1_MIN_COLS sends to the bf16x1 kernel at `lane_frames` frames of 96x160 per lane
    (csrc/trunk_route.h: choose_route): 1x1, stride 1, Cin % 16 == 0 and lane_frames x (pixels of the conv's map) >= min_cols.  Bottleneck trunks: conv3 and
    layer1's downsample (Cout = 4 Cin) and the conv1 of later blocks (Cin = 4 Cout) run on their stage's map, the conv1 of a stage's first block
    (Cin = 2 Cout, or 64 -> 64) on the stage before's."""
    from frtm_vos_amd import _hip as H
    info = (ctypes.c_int * 6)()
    out = []
    for i in range(_lib().frtm_backbone_num_convs(ext._handle)):
        H.call_nostream('frtm_backbone_conv_info', ext._handle, i, info)
        cout, cin, k, s = info[0], info[1], info[2], info[3]
        if k != 1 or s != 1 or cin % 16:
            continue
        if cout == 4 * cin:
            stage = (cin // 64).bit_length() - 1
        elif cin == 4 * cout:
            stage = (cout // 64).bit_length() - 1
        elif cin == 2 * cout:
            stage = (cout // 64).bit_length() - 2
        else:
            assert cin == cout == 64, (cin, cout)
            stage = 0
        if lane_frames * HW[stage] >= min_cols:
            out.append(i)
    return out


@pytest.fixture(scope='module')
def trunk():
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    ext = _with_min_cols(lambda: ResnetFeatureExtractor('resnet50', seed=0).to(DEV))
    img = torch.randint(0, 256, (4, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(11)).to(DEV)
    ext.lanes = 1
    return ext, img, {k: v.clone() for k, v in ext(img).items()}


def _pass(ext, img, **kw):
    L = _lib()
    a = L.frtm_conv_bf16x1_launches()
    taps = {k: v.clone() for k, v in ext(img, **kw).items()}
    torch.cuda.synchronize()
    return taps, L.frtm_conv_bf16x1_launches() - a


def test_trunk_routing_counts_round_trip_lanes_and_plan(trunk):
    from frtm_vos_amd import _hip as H
    L = _lib()
    ext, img, t0 = trunk
    # layer1 (7 convs) and layer2 (8) at 2 and 4 frames per lane, and the conv1 of layer3's first block (on layer2's map); at 1 frame layer1 and the
    # conv1 of layer2's first block only
    assert len(routed_convs(ext, 4)) == 16 and len(routed_convs(ext, 2)) == 16 and len(routed_convs(ext, 1)) == 8
    b3 = L.frtm_conv_bf16x3_launches()
    try:
        ext.lanes = 1
        f32, n = _pass(ext, img)
        assert n == 0 and all(torch.equal(f32[k], t0[k]) for k in t0)
        ext.precision = 'bf16x1'
        assert ext.precision == 'bf16x1'
        t1, n = _pass(ext, img)
        assert n == len(routed_convs(ext, 4)), n                      # one lane of 4 frames
        for k in t1:
            assert bool(torch.isfinite(t1[k]).all()), k
            rel = float((t1[k] - t0[k]).abs().max() / t0[k].abs().max())
            print('%s: bf16x1 taps against fp32 taps, max |diff| / max |fp32| = %.3e' % (k, rel))
        assert all(not torch.equal(t1[k], t0[k]) for k in ('layer2', 'layer3', 'layer4', 'layer5'))
        # two lanes of 2 frames equal one lane per half, bit for bit; every lane runs every routed conv of its frames
        ext.lanes = 2
        t2, n = _pass(ext, img)
        assert n == 2 * len(routed_convs(ext, 2)), n
        t2s1, n = _pass(ext, img, lane_set=1)
        assert n == 2 * len(routed_convs(ext, 2)), n
        ext.lanes = 1
        ha, n = _pass(ext, img[:2])
        assert n == len(routed_convs(ext, 2)), n
        hb, _ = _pass(ext, img[2:])
        for k in t2:
            assert torch.equal(torch.cat([ha[k], hb[k]]), t2[k]), k
            assert torch.equal(t2s1[k], t2[k]), k
        # a conv plan keeps its conv on fp32
        idx = routed_convs(ext, 4)[3]
        H.call_nostream('frtm_backbone_set_conv_plan', ext._handle, idx, 1, 0)
        try:
            _, n = _pass(ext, img)
            assert n == len(routed_convs(ext, 4)) - 1, n
        finally:
            H.call_nostream('frtm_backbone_set_conv_plan', ext._handle, idx, 0, 0)
        # bf16x3 and back: the modes are exclusive (at this size the bf16x3 router picks nothing, so its taps are the fp32 ones)
        ext.precision = 'bf16x3'
        t3, n = _pass(ext, img)
        assert n == 0 and all(torch.equal(t3[k], t0[k]) for k in t0)
        ext.precision = 'bf16x1'
        t1b, n = _pass(ext, img)
        assert n == len(routed_convs(ext, 4)) and all(torch.equal(t1b[k], t1[k]) for k in t1)
        with pytest.raises(ValueError):
            ext.precision = 'bf16'
        with pytest.raises(RuntimeError):
            H.call_nostream('frtm_backbone_set_bf16_pieces', ext._handle, 2)
        assert ext.precision == 'bf16x1'
        _, n = _pass(ext, img)
        assert n == len(routed_convs(ext, 4))                          # the rejected calls left the mode as it was
        # back to fp32: bit-identical to before
        ext.precision = 'fp32'
        f32b, n = _pass(ext, img)
        assert n == 0 and all(torch.equal(f32b[k], t0[k]) for k in t0)
        assert L.frtm_conv_bf16x3_launches() == b3                     # a bf16x1 trunk never launches the bf16x3 kernel
    finally:
        ext.precision = 'fp32'
        ext.lanes = 1


def test_trunk_vs_oracle_is_printed_not_gated():
    """Taps of the bf16x1 trunk against the CPU oracle, per tap, next to the fp32 trunk's: printed (and recorded at full size in
    profiles/bf16x1_trunk_time.txt).  No numeric gate: the figure cannot be derived, and it must not be set from the code under test."""
    from oracle import cpu_ref as O
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    P = O.resnet_random_params('resnet50', seed=3)
    img = torch.randint(0, 256, (4, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    ref = O.resnet_forward('resnet50', P, img)
    ext = _with_min_cols(lambda: ResnetFeatureExtractor('resnet50', weights=P).to(DEV))
    ext.lanes = 1
    out = {}
    for mode in ('fp32', 'bf16x1'):
        ext.precision = mode
        out[mode], n = _pass(ext, img.to(DEV))
        assert n == (len(routed_convs(ext, 4)) if mode == 'bf16x1' else 0)
    for k in sorted(ref):
        e = [float((out[m][k].double().cpu() - ref[k].double()).abs().max() / (ref[k].double().abs().max() + 1e-30)) for m in ('fp32', 'bf16x1')]
        print('resnet50 B=4 %s: rel err against the oracle fp32 %.3e bf16x1 %.3e' % (k, e[0], e[1]))
        assert bool(torch.isfinite(out['bf16x1'][k]).all()), k


# (Cin, Cout) -> fewest columns per launch from which trunk_route.h's kTrunkRules routes the shape (profiles/bf16x1_trunk_time.txt)
DEFAULT_RULES = {(256, 1024): 1620, (1024, 256): 1620, (128, 512): 6420, (512, 128): 6420, (512, 2048): 405, (2048, 512): 3240, (256, 64): 25680}


def default_table_count(cols):
    """Launches per ResNet-50 pass in one lane under DEFAULT_RULES; cols[s] = columns (frames x pixels) of stage s's map.  Blocks per stage 3, 4, 6, 3:
    the conv3 shape (64 << s) -> (256 << s) runs once per block (layer1's downsample has the same shape: one more), the conv1 shape
    (256 << s) -> (64 << s) in every block but the stage's first; the first blocks' conv1 shapes are in no rule."""
    blocks = (3, 4, 6, 3)
    n = 0
    for s in range(4):
        c = 64 << s
        if DEFAULT_RULES.get((c, 4 * c), 1 << 62) <= cols[s]:
            n += blocks[s] + (1 if s == 0 else 0)
        if DEFAULT_RULES.get((4 * c, c), 1 << 62) <= cols[s]:
            n += blocks[s] - 1
    return n


def test_default_router_table():
    """Without the knob the router's table holds column counts measured on 480x854 frames.  One such frame: every measured shape but layer1's
    64 -> 256 and layer4's 2048 -> 512 is routed; two frames of 96x160 (at most 1920 columns) route nothing and the taps are the fp32 ones."""
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    ext = ResnetFeatureExtractor('resnet50', seed=0).to(DEV)
    big = torch.randint(0, 256, (1, 3, 480, 854), dtype=torch.uint8, generator=torch.Generator().manual_seed(12)).to(DEV)
    small = torch.randint(0, 256, (2, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(13)).to(DEV)
    f32, _ = _pass(ext, small)
    ext.precision = 'bf16x1'
    want = default_table_count({0: 120 * 214, 1: 60 * 107, 2: 30 * 54, 3: 15 * 27})
    assert want == 2 + 4 + 3 + 6 + 5 + 3
    taps, n = _pass(ext, big)
    assert n == want, n
    assert all(bool(torch.isfinite(v).all()) for v in taps.values())
    taps, n = _pass(ext, small)
    assert n == default_table_count({s: 2 * HW[s] for s in HW}) == 0, n
    assert all(torch.equal(taps[k], f32[k]) for k in f32)


# ---- 7. BasicBlock trunks have no stride-1 1x1 conv: nothing is routed even when every eligible conv would be
def test_resnet18_routes_nothing():
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    ext = _with_min_cols(lambda: ResnetFeatureExtractor('resnet18', seed=2).to(DEV), 0)
    img = torch.randint(0, 256, (2, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(6)).to(DEV)
    a, _ = _pass(ext, img)
    ext.precision = 'bf16x1'
    b, n = _pass(ext, img)
    assert n == 0
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 8. graphs
def test_graph_recaptured_on_precision_switch(trunk):
    ext, img, t0 = trunk
    ext.lanes = 1
    ext.precision = 'bf16x1'
    eager, _ = _pass(ext, img)
    ext.precision = 'fp32'
    ext.reuse_outputs, ext.use_graph = True, True
    try:
        for _ in range(3):
            f32 = ext(img)
        f32 = {k: v.clone() for k, v in f32.items()}
        assert any(e['graph'] is not None for e in ext._out_cache.values())
        ext.precision = 'bf16x1'
        assert not ext._out_cache
        for _ in range(3):
            out = ext(img)
        torch.cuda.synchronize()
        assert any(e['graph'] is not None for e in ext._out_cache.values())
        for k in eager:
            assert torch.equal(out[k], eager[k]), k
            assert torch.equal(f32[k], t0[k]), k
        assert any(not torch.equal(out[k], f32[k]) for k in eager)
    finally:
        ext.reuse_outputs, ext.use_graph = False, False
        ext.precision = 'fp32'
        ext._out_cache.clear()


# ---- 9. tracker plumbing
def test_tracker_runs_with_a_bf16x1_trunk():
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    torch.set_grad_enabled(False)
    L = _lib()
    seq = SyntheticSequence('bf16x1', 6, (128, 160), 2, seed=31)
    seq.preload(DEV)
    labels = {}
    for mode in ('fp32', 'bf16x1'):
        torch.manual_seed(0)
        params = Parameters(None, device=DEV, feature_extractor='resnet50', trunk_precision=mode)
        trk = _with_min_cols(lambda: params.get_model().eval(), 0)          # every eligible conv of the bf16x1 trunk is routed
        assert trk.feature_extractor.precision == mode
        a = L.frtm_conv_bf16x1_launches()
        out, _ = trk.run_sequence(seq)
        torch.cuda.synchronize()
        moved = L.frtm_conv_bf16x1_launches() - a
        assert (moved > 0) == (mode == 'bf16x1'), (mode, moved)
        assert len(out) == 6
        for lb in out:
            assert set(int(v) for v in lb.unique().tolist()) <= {0, 1, 2}
        labels[mode] = torch.stack([lb.cpu() for lb in out])
    agree = float((labels['fp32'] == labels['bf16x1']).float().mean())
    print('label agreement of the bf16x1 tracker with the fp32 tracker over 6 frames: %.4f (not gated)' % agree)
