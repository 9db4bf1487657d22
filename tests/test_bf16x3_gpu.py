"""The bf16x3 trunk mode on the GPU: the FRTM_WLAYOUT_BF16X3 1x1 kernel (csrc/conv_bf16x3.hip) exactly, against fp64 on trunk data, its determinism,
the trunk's routing, the trunk against the oracle, graph re-capture and a tracker run with a bf16x3 trunk.

Exact cases: every operand is one of +-1, +-(1 + 2^-9), +-(1 + 2^-9 + 2^-18) or 0, whose three bf16 pieces are exactly 1, 2^-9 and 2^-18.  Which of them
a weight or an activation may take depends on k % 3, so that for every k the three piece products the kernel drops (mid.lo, lo.mid, lo.lo) are zero
while, over the k, each of the six it forms carries weight (k % 3 == 0: weight hi only against any activation -> hi.lo; k % 3 == 1: hi + mid against
hi + mid -> mid.mid; k % 3 == 2: any weight against activation hi only -> lo.hi).  With at most 16 non-zero weights per output row, every partial sum
is a multiple of 2^-18 below 2^5, and the epilogue (power-of-two scale, quarter-step shift and residual) keeps it within fp32's 24 bits: the output
must equal an fp64 convolution BIT FOR BIT.  A dropped or mis-indexed piece product moves outputs by 2^-9 or 2^-18.  Buffers are framed as in
tests/test_conv_forms_gpu.py: NaN-filled outputs between sentinel bands, NaN-framed inputs and residuals."""
import ctypes
import itertools

import pytest
import torch

from oracle import cpu_ref as O
from test_conv_forms_gpu import Framed, _nan_framed

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1500)]

DEV = 'cuda'
BF16X3 = 5
VALUES = (1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9 + 2.0 ** -18)       # pieces: (1), (1, 2^-9), (1, 2^-9, 2^-18)
W_TYPES = {0: 1, 1: 2, 2: 3}                                          # k % 3 -> how many of VALUES a weight may take
X_TYPES = {0: 3, 1: 2, 2: 1}


def _lib():
    from frtm_vos_amd import _hip as H
    return H.lib()


def _last():
    return _lib().frtm_conv_last_kernels().decode()


def _typed(g, shape, kaxis, types):
    """Values from VALUES (times a random sign), or 0, with the allowed count of VALUES chosen by the k index along `kaxis`."""
    k = torch.arange(shape[kaxis]).view([-1 if i == kaxis else 1 for i in range(len(shape))]).expand(shape)
    allowed = torch.tensor([types[i % 3] for i in range(3)])[k % 3]
    pick = (torch.rand(shape, generator=g) * allowed.float()).long()
    v = torch.tensor(VALUES, dtype=torch.float64)[pick]
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    keep = torch.rand(shape, generator=g) < 0.8
    return (v * sign * keep).float()


def exact_operands(g, B, cin, cout, h, w):
    x = _typed(g, (B, cin, h, w), 1, X_TYPES)
    wt = _typed(g, (cout, cin), 1, W_TYPES)
    period = max(1, (cin + 15) // 16)                                  # at most 16 non-zero weights per output channel
    m, k = torch.meshgrid(torch.arange(cout), torch.arange(cin), indexing='ij')
    wt = wt * (((m + k) % period) == 0).float()
    return x, wt.view(cout, cin, 1, 1)


def bf_case(B, cin, cout, h, w, scale=False, res=False, relu=False, seed=0):
    """One FRTM_WLAYOUT_BF16X3 call on framed buffers; asserts the kernels, the guard bands and the exact result."""
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(seed * 7919 + B * 1009 + cin * 101 + cout * 11 + h + w)
    x, wt = exact_operands(g, B, cin, cout, h, w)
    sc = (2.0 ** torch.randint(-1, 2, (cout,), generator=g)) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1)
    sh = torch.randint(-8, 9, (cout,), generator=g) / 4.0
    rs = torch.randint(-8, 9, (B, cout, h, w), generator=g) / 4.0
    wB, _, lay = ops.pack_weights(wt.to(DEV), bf16x3=True)
    assert lay == BF16X3 and _last() == 'k_pack_weights_bf16x3'
    out = Framed(B * cout * h * w)
    out.view.fill_(float('nan'))
    ops.conv2d(_nan_framed(x), wB, cout, 1, 1, 0, scale=sc.float().to(DEV) if scale else None, shift=sh.float().to(DEV) if scale else None,
               residual=_nan_framed(rs.float()) if res else None, relu=relu, out=out.view.view(B, cout, h, w), w_layout=BF16X3)
    assert _last() == 'k_conv1x1_bf16x3'
    torch.cuda.synchronize()
    label = (B, cin, cout, h, w, scale, res, relu)
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
@pytest.mark.parametrize('B,cin,cout,h,w', [
    (2, 48, 65, 6, 10),        # Cout tail, three K chunks (an odd count: both LDS stages), one pixel tile across both images
    (1, 16, 130, 11, 13),      # B = 1, one K chunk, two Cout tiles (the second with 2 rows), 143 pixels (odd, ragged tile)
    (8, 64, 256, 15, 27),      # B = 8 on the layer4 map size (405 pixels: tiles straddle images), Cout multiple of the tile
    (3, 32, 33, 7, 9),
    (8, 256, 96, 4, 5),        # 256-deep K, 20-pixel images: a tile spans seven images
])
def test_exact_shapes(B, cin, cout, h, w):
    bf_case(B, cin, cout, h, w, scale=True, res=True, relu=True)


@pytest.mark.parametrize('scale,res,relu', list(itertools.product((False, True), repeat=3)))
def test_exact_every_epilogue(scale, res, relu):
    bf_case(2, 80, 72, 9, 7, scale=scale, res=res, relu=relu, seed=1)


def test_exact_case_needs_every_piece_product():
    """The data of the exact cases carries weight in each of the six products: the fp64 sum over only five of them differs somewhere."""
    g = torch.Generator().manual_seed(3)
    x, wt = exact_operands(g, 2, 48, 65, 6, 10)

    def pieces(t):
        t = t.double()
        hi = t.sign() * (t.abs() >= 1).double()
        mid = t.sign() * ((t.abs() - 1) >= 2.0 ** -9).double() * 2.0 ** -9
        return hi, mid, t - hi - mid
    W, X = pieces(wt.view(65, 48)), pieces(x.view(2, 48, -1))
    prods = [(0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0)]
    full = sum(torch.einsum('mk,bkp->bmp', W[a], X[b]) for a, b in prods)
    exact = torch.einsum('mk,bkp->bmp', wt.double().view(65, 48), x.double().view(2, 48, -1))
    assert torch.equal(full, exact)                                     # the dropped products are zero on this data
    for drop in prods:
        part = sum(torch.einsum('mk,bkp->bmp', W[a], X[b]) for a, b in prods if (a, b) != drop)
        assert not torch.equal(part, exact), drop


# ---- 2. error bound on trunk data
@pytest.fixture(scope='module')
def trunk():
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    ext = ResnetFeatureExtractor('resnet101', seed=0).to(DEV)
    ext.lanes = 2
    img = torch.randint(0, 256, (8, 3, 480, 854), dtype=torch.uint8, generator=torch.Generator().manual_seed(11)).to(DEV)
    return ext, img, ext(img)


def _folded(cv, bn):
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).float()
    return cv.weight.data.float().to(DEV), scale.to(DEV), (bn.bias - bn.running_mean * scale).float().to(DEV)


def trunk_operands(ext, taps, name):
    """(x, w) of one stride-1 1x1 trunk shape: the stage's tap, through conv1 + BN + ReLU of the stage's block 1 for the narrow inputs."""
    from frtm_vos_amd import ops
    R = ext.resnet
    tap, blk = {'256->1024': ('layer4', R.layer3[1]), '1024->256': ('layer4', R.layer3[2]), '64->256': ('layer2', R.layer1[1]),
                '128->512': ('layer3', R.layer2[1]), '512->2048': ('layer5', R.layer4[1])}[name]
    w1, s1, b1 = _folded(blk.conv1, blk.bn1)
    if name == '1024->256':
        return taps[tap], w1
    wp, kt, _ = ops.pack_weights(w1)
    x = ops.conv2d(taps[tap], wp, w1.shape[0], 1, 1, 0, ktab=kt, scale=s1, shift=b1, relu=True)
    return x, _folded(blk.conv3, blk.bn3)[0]


@pytest.mark.parametrize('name', ['256->1024', '1024->256', '64->256', '128->512', '512->2048'])
def test_error_within_1p5x_of_fp32(trunk, name):
    from frtm_vos_amd import ops
    ext, _, taps = trunk
    x, w = trunk_operands(ext, taps, name)
    B, cin = x.shape[0], x.shape[1]
    cout = w.shape[0]
    wT, kt, lay = ops.pack_weights(w)
    wB, _, _ = ops.pack_weights(w, bf16x3=True)
    g32 = ops.conv2d(x, wT, cout, 1, 1, 0, ktab=kt, w_layout=lay).double().reshape(B, cout, -1)
    gb = ops.conv2d(x, wB, cout, 1, 1, 0, w_layout=BF16X3)
    assert _last() == 'k_conv1x1_bf16x3'
    gb = gb.double().reshape(B, cout, -1)
    ref = torch.matmul(w.double().reshape(cout, cin), x.double().reshape(B, cin, -1))
    e32, eb = (g32 - ref).abs(), (gb - ref).abs()
    m32, mb, r32, rb = float(e32.max()), float(eb.max()), float(e32.pow(2).mean().sqrt()), float(eb.pow(2).mean().sqrt())
    print('%s: max err fp32 %.3e bf16x3 %.3e (%.2fx), rms %.3e / %.3e (%.2fx)' % (name, m32, mb, mb / m32, r32, rb, rb / r32))
    assert mb <= 1.5 * m32 and rb <= 1.5 * r32, (name, m32, mb, r32, rb)


# ---- 3. determinism
def test_two_launches_bit_identical(trunk):
    from frtm_vos_amd import ops
    ext, _, taps = trunk
    x, w = trunk_operands(ext, taps, '256->1024')
    wB, _, _ = ops.pack_weights(w, bf16x3=True)
    a = ops.conv2d(x, wB, w.shape[0], 1, 1, 0, w_layout=BF16X3, relu=True)
    b = ops.conv2d(x, wB, w.shape[0], 1, 1, 0, w_layout=BF16X3, relu=True)
    assert torch.equal(a, b)
    # a sub-batch computes the same columns bit for bit (other grid size, other tile boundaries)
    c = ops.conv2d(x[3:5].contiguous(), wB, w.shape[0], 1, 1, 0, w_layout=BF16X3, relu=True)
    assert torch.equal(c, a[3:5])


def test_trunk_taps_independent_of_lanes_and_lane_set(trunk):
    """Two lanes of 4 frames against one lane per 4 frames, and lane set 1 against lane set 0.  (The fp32 planner picks its tiles, split-K and
    Winograd forms by the frames of a lane, so one lane of 16 frames is not the reference here.)"""
    ext, img, _ = trunk
    ext.precision = 'bf16x3'
    try:
        img16 = torch.cat([img, img.roll(7, dims=3)])          # 8 frames per lane: layer4's conv3 is routed in each
        ext.lanes = 2
        t2 = {k: v.clone() for k, v in ext(img16).items()}
        t2s1 = {k: v.clone() for k, v in ext(img16, lane_set=1).items()}
        ext.lanes = 1
        t1 = {k: v.clone() for k, v in ext(img16[:8]).items()}
        t1b = ext(img16[8:])
        for k in t1:
            assert torch.equal(torch.cat([t1[k], t1b[k]]), t2[k]), k
            assert torch.equal(t2s1[k], t2[k]), k
    finally:
        ext.lanes = 2
        ext.precision = 'fp32'


# ---- 4. routing
def _desc(**kw):
    from frtm_vos_amd import _hip as H
    d = dict(B=1, Cin=32, Hin=8, Win=8, Cout=32, ksize=1, stride=1, pad=0, relu=0, out_transposed=0, splitk=0, tile=0, w_layout=BF16X3, ws_elems=0,
             w_pitch=0)
    d.update(kw)
    return H.ConvDesc(*[d[k] for k, _ in H.ConvDesc._fields_])


@pytest.mark.parametrize('bad', [dict(ksize=3, pad=1), dict(stride=2), dict(pad=1, ksize=1), dict(out_transposed=1), dict(w_pitch=32), dict(Cin=40),
                                 dict(tile=1), dict(splitk=2)])
def test_ineligible_descriptors_are_argument_errors(bad):
    L = _lib()
    x = torch.zeros(1 << 16, device=DEV)
    wB = torch.zeros(1 << 16, device=DEV)
    out = torch.zeros(1 << 16, device=DEV)
    d = _desc(**bad)
    before = L.frtm_conv_bf16x3_launches()
    rc = L.frtm_conv2d(ctypes.byref(d), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(wB.data_ptr()), None, None, None, None,
                       ctypes.c_void_p(out.data_ptr()), None, None)
    assert rc == -1, (bad, rc)
    assert L.frtm_conv_bf16x3_launches() == before and _last() == ''
    assert b'frtm_conv2d' in L.frtm_last_error()


def test_ineligible_pack_is_an_argument_error():
    L = _lib()
    w = torch.zeros(64 * 40 * 9, device=DEV)
    out = torch.zeros(1 << 16, device=DEV)
    for cin, k in ((40, 1), (32, 3)):
        rc = L.frtm_conv_pack_weights(ctypes.c_void_p(w.data_ptr()), 64, cin, k, BF16X3, ctypes.c_void_p(out.data_ptr()), None, None)
        assert rc == -1, (cin, k)


def routed_convs(ext, lane_frames=8, hw=405):
    """Indices of the convs a bf16x3 trunk sends to the bf16x3 kernel at `lane_frames` frames per lane of 480x854 (csrc/trunk_route.h: kTrunkRules:
    layer4's 512 -> 2048 conv3 with >= 3240 columns; hw = its 15x27 map)."""
    from frtm_vos_amd import _hip as H
    info = (ctypes.c_int * 6)()
    out = []
    for i in range(_lib().frtm_backbone_num_convs(ext._handle)):
        H.call_nostream('frtm_backbone_conv_info', ext._handle, i, info)
        cout, cin, k, s = info[0], info[1], info[2], info[3]
        if k == 1 and s == 1 and cin == 512 and cout == 2048 and lane_frames * hw >= 3240:
            out.append(i)
    return out


def test_launch_count_per_pass_and_round_trip(trunk):
    L = _lib()
    ext, img, _ = trunk
    n = len(routed_convs(ext))
    assert n == 3 and routed_convs(ext, 4) == []     # layer4's three conv3 at 8 frames per lane, none at 4
    ext.precision = 'fp32'
    a = L.frtm_conv_bf16x3_launches()
    t0 = {k: v.clone() for k, v in ext(img).items()}
    torch.cuda.synchronize()
    assert L.frtm_conv_bf16x3_launches() == a
    ext.precision = 'bf16x3'
    img16 = torch.cat([img, img])
    for lanes, x, want in ((2, img, 0), (2, img16, 2 * n), (1, img, n)):        # every lane runs every routed conv of its frames
        ext.lanes = lanes
        a = L.frtm_conv_bf16x3_launches()
        tb = ext(x)
        torch.cuda.synchronize()
        assert L.frtm_conv_bf16x3_launches() - a == want, (lanes, x.shape[0])
    ext.lanes = 2
    assert any(not torch.equal(tb[k], t0[k]) for k in ('layer3', 'layer4', 'layer5'))
    ext.precision = 'fp32'
    a = L.frtm_conv_bf16x3_launches()
    t1 = ext(img)
    torch.cuda.synchronize()
    assert L.frtm_conv_bf16x3_launches() == a
    for k in t0:
        assert torch.equal(t0[k], t1[k]), k


def test_plan_override_keeps_the_conv_fp32(trunk):
    from frtm_vos_amd import _hip as H
    L = _lib()
    ext, img, _ = trunk
    idx = routed_convs(ext)[1]
    ext.precision = 'bf16x3'
    ext.lanes = 1
    try:
        H.call_nostream('frtm_backbone_set_conv_plan', ext._handle, idx, 1, 0)
        a = L.frtm_conv_bf16x3_launches()
        ext(img)
        torch.cuda.synchronize()
        assert L.frtm_conv_bf16x3_launches() - a == len(routed_convs(ext)) - 1
    finally:
        H.call_nostream('frtm_backbone_set_conv_plan', ext._handle, idx, 0, 0)
        ext.precision = 'fp32'
        ext.lanes = 2


def test_precision_setter_validates(trunk):
    ext = trunk[0]
    with pytest.raises(ValueError):
        ext.precision = 'bf16'
    assert ext.precision == 'fp32'
    with pytest.raises(RuntimeError):
        from frtm_vos_amd import _hip as H
        H.call_nostream('frtm_backbone_set_precision', ext._handle, 2)


# ---- 5. trunk against the oracle
def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize('name', ['resnet101', 'resnet50'])
def test_trunk_vs_oracle(name):
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    P = O.resnet_random_params(name, seed=3)
    img = torch.randint(0, 256, (8, 3, 480, 854), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    ref = O.resnet_forward(name, P, img)
    ext = ResnetFeatureExtractor(name, weights=P, precision='bf16x3').to(DEV)
    ext.lanes = 1                                    # 8 frames in one lane: layer4's conv3 is routed (at B = 1 nothing is)
    for B in (8, 1):
        ext.precision = 'fp32'
        f32 = {k: v.cpu() for k, v in ext(img[:B].to(DEV)).items()}
        ext.precision = 'bf16x3'
        bf = {k: v.cpu() for k, v in ext(img[:B].to(DEV)).items()}
        for L in ref:
            e32, eb = _rel(f32[L], ref[L][:B]), _rel(bf[L], ref[L][:B])
            print('%s B=%d %s: rel err fp32 %.3e bf16x3 %.3e' % (name, B, L, e32, eb))
            assert eb < 2e-4, (name, B, L, eb)
            assert eb <= 1.5 * e32 + 1e-7, (name, B, L, e32, eb)


def test_resnet18_routes_nothing():
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    L = _lib()
    ext = ResnetFeatureExtractor('resnet18', seed=2).to(DEV)
    img = torch.randint(0, 256, (2, 3, 240, 432), dtype=torch.uint8, generator=torch.Generator().manual_seed(6)).to(DEV)
    a = {k: v.clone() for k, v in ext(img).items()}
    ext.precision = 'bf16x3'
    n = L.frtm_conv_bf16x3_launches()
    b = ext(img)
    torch.cuda.synchronize()
    assert L.frtm_conv_bf16x3_launches() == n
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 6. graphs
def test_graph_recaptured_on_precision_switch(trunk):
    ext, img, _ = trunk
    ext.lanes = 1                                    # 8 frames in one lane: layer4's conv3 is routed
    ext.precision = 'bf16x3'
    eager = {k: v.clone() for k, v in ext(img).items()}
    ext.precision = 'fp32'
    ext.reuse_outputs, ext.use_graph = True, True
    try:
        for _ in range(3):
            f32 = ext(img)
        f32 = {k: v.clone() for k, v in f32.items()}
        assert any(e['graph'] is not None for e in ext._out_cache.values())
        ext.precision = 'bf16x3'
        assert not ext._out_cache
        for _ in range(3):
            out = ext(img)
        torch.cuda.synchronize()
        assert any(e['graph'] is not None for e in ext._out_cache.values())
        for k in eager:
            assert torch.equal(out[k], eager[k]), k
        assert any(not torch.equal(out[k], f32[k]) for k in eager)
    finally:
        ext.reuse_outputs, ext.use_graph = False, False
        ext.precision = 'fp32'
        ext.lanes = 2
        ext._out_cache.clear()


# ---- 7. tracker
def test_tracker_teacher_forced_with_bf16x3_trunk(monkeypatch):
    import oracle.make_golden_jf as JF
    from frtm_vos_amd.evaluate import Parameters
    from test_north_star_gpu import _teacher_forced
    d = list(Parameters.__init__.__defaults__)
    i = Parameters.__init__.__code__.co_varnames[1:Parameters.__init__.__code__.co_argcount].index('trunk_precision') - (
        Parameters.__init__.__code__.co_argcount - 1 - len(d))
    d[i] = 'bf16x3'
    monkeypatch.setattr(Parameters.__init__, '__defaults__', tuple(d))
    assert Parameters(None).trunk_precision == 'bf16x3'
    # A PLUMBING check: the mode reaches the tracker's extractor and leaves its results within the north star's bars.  The teacher-forced run's
    # trunk passes (5 augmented frames, then one frame per track()) are below the router's 8 frames per lane, so no conv goes
    # to the bf16x3 kernel here -- asserted, so that a router change that starts routing them makes this test exercise the kernel knowingly.
    # The kernel itself is covered by the exact, error-bound and trunk tests above.
    L = _lib()
    n = L.frtm_conv_bf16x3_launches()
    worst = _teacher_forced(JF.SIZE, 18, 2, 300, dict(JF.DISC))
    assert L.frtm_conv_bf16x3_launches() == n
    assert worst['raw'] <= 1e-3, worst
    assert worst['merged'] <= 1e-3, worst
    assert worst['arb'] <= 1.5, worst
