"""The bf16x1_act trunk mode on the GPU.  Every comparison is BIT FOR BIT: the format-aware kernels of csrc/conv_bf16act.hip keep their parent
kernel's K loop, so each result is an exact function of the parent's result (include/frtm_hip.h: frtm_conv2d_act) --

    bf16 input      ->  the parent's result y0 (the parent rounds its fp32 input to bf16 anyway)
    bf16 residual   ->  parent(x, r.bfloat16().float())
    bf16 output     ->  act_to_bf16(y0'), y0' the fp32-output result of the same input and residual formats

-- and the trunk under the mode equals a Python walk of its blocks through ops.conv2d in fp32 NCHW with t.bfloat16().float() applied to exactly the
tensors frtm_backbone_act_plan marks.  Only the comparison with fp64 (section 7) has a margin, the parent mode's rule.
Buffers are framed by bands of a sentinel NaN pattern no kernel produces, sized for the half-size bf16 buffers; operands hold no NaN and no denormal."""
import ctypes
import itertools
import os

import pytest
import torch
from torch.nn import functional as F

from _bf16act_refs import Trunk

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = 'cuda'
GUARD = 256                   # 32-bit words of guard band on each side (a multiple of 4: the framed tensors keep 16-byte alignment)
SENT = 0x7FA5A5A5             # sentinel word (a NaN pattern no kernel produces)
L1, S1, S2 = 6, 7, 8          # FRTM_WLAYOUT_BF16X1, _BF16X1_3X3, _BF16X1_3X3_S2
# kind -> (layout, ksize, stride, pad, kernel name per (tile, in_fmt), the parent's kernel per tile)
KINDS = {
    '1x1': (L1, 1, 1, 0, {1: 'k_conv1x1_act<128,64,64,%d>', 2: 'k_conv1x1_act<64,64,64,%d>'}, {1: 'k_conv1x1_bf16x1<128,64,64>', 2: 'k_conv1x1_bf16x1<64,64,64>'}),
    '3x3': (S1, 3, 1, 1, {1: 'k_conv3x3_act<2,%d>', 2: 'k_conv3x3_act<3,%d>'}, {1: 'k_conv3x3_bf16x1<2>', 2: 'k_conv3x3_bf16x1<3>'}),
    '3x3s2': (S2, 3, 2, 1, {1: 'k_conv3x3s2_act<2,%d>', 2: 'k_conv3x3s2_act<3,%d>'}, {1: 'k_conv3x3s2_bf16x1<2>', 2: 'k_conv3x3s2_bf16x1<3>'}),
}
SHAPES = {     # (B, Cin, Cout, H, W)
    '1x1': [(2, 80, 72, 15, 27),       # a K tail of 16 after one chunk of 64, Cout no multiple of a tile, 405 columns per image: tiles straddle images
            (1, 16, 8, 1, 3),
            (3, 128, 136, 5, 7)],
    '3x3': [(2, 24, 40, 15, 27),       # Cin % 16 == 8: the last chunk's second slice is absent
            (2, 64, 64, 9, 35),        # crosses the 8-row and 32-column tile edges
            (1, 16, 8, 1, 1)],
    '3x3s2': [(2, 24, 40, 15, 27),     # -> 8 x 14
              (1, 64, 128, 30, 54),
              (2, 16, 8, 2, 2)],
}


def _lib():
    from frtm_vos_amd import _hip as H
    return H.lib()


def _last():
    return _lib().frtm_conv_last_kernels().decode()


def _counts():
    """(1x1, layout 7, layout 8, format-aware) launches"""
    L = _lib()
    return L.frtm_conv_bf16x1_launches(), L.frtm_conv_bf16x1_3x3_launches(), L.frtm_conv_bf16x1_3x3s2_launches(), L.frtm_conv_bf16act_launches()


class Framed:
    """A tensor of `numel` elements of `dtype` (4 or 2 bytes each, a multiple of 4 bytes in all) between two guard bands of sentinel words."""

    def __init__(self, numel, dtype=torch.float32):
        nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        assert nbytes % 4 == 0
        self.words = nbytes // 4
        self.buf = torch.empty(self.words + 2 * GUARD, device=DEV, dtype=torch.int32)
        self.buf.fill_(SENT)
        self.view = self.buf[GUARD:GUARD + self.words].view(dtype)
        assert self.view.numel() == numel and self.view.data_ptr() % 16 == 0

    def put(self, t):
        self.view.copy_(t.reshape(-1))
        return self

    def reset(self):
        self.buf.fill_(SENT)
        return self

    def intact(self):
        return bool((self.buf[:GUARD] == SENT).all()) and bool((self.buf[GUARD + self.words:] == SENT).all())


def _operands(kind, B, cin, cout, h, w, seed=0):
    _, k, stride, pad = KINDS[kind][:4]
    g = torch.Generator().manual_seed(seed * 7919 + B * 1009 + cin * 101 + cout * 11 + h + w)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    x = torch.randn(B, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, k, k, generator=g) / (k * k * cin) ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g) * 0.1
    rs = torch.randn(B, cout, ho, wo, generator=g)
    return x, wt, sc, sh, rs, (ho, wo)


class Case:
    """One conv shape on the device: framed operands in both formats, the packed image, and a framed launch."""

    def __init__(self, kind, B, cin, cout, h, w, seed=0, x=None):
        from frtm_vos_amd import ops
        self.kind, self.dims = kind, (B, cin, cout, h, w)
        self.layout, self.k, self.stride, self.pad, self.names, self.parents = KINDS[kind]
        x0, wt, sc, sh, rs, self.out_hw = _operands(kind, B, cin, cout, h, w, seed)
        x0 = x0 if x is None else x
        self.x_cpu, self.wt_cpu = x0, wt
        self.wT = ops.pack_weights(wt.to(DEV), bf16x1=True, stride=self.stride)[0]
        self.sc, self.sh = sc.to(DEV), sh.to(DEV)
        n_in, n_out = x0.numel(), rs.numel()
        self.x = {0: Framed(n_in).put(x0.to(DEV)), 1: Framed(n_in, torch.bfloat16).put(ops.act_to_bf16(x0.to(DEV)))}
        self.r = {'f32': Framed(n_out).put(rs.to(DEV)), 'bf16': Framed(n_out, torch.bfloat16).put(ops.act_to_bf16(rs.to(DEV))),
                  'rounded': Framed(n_out).put(rs.to(DEV).bfloat16().float())}
        self.out = {0: Framed(n_out), 1: Framed(n_out, torch.bfloat16)}

    def run(self, tile, in_fmt, res, out_fmt, scale, relu):
        """res: None, 'f32', 'bf16', or 'rounded' (fp32 format, the bf16 values).  -> a clone of the output: (B,Cout,Ho,Wo) fp32, or the flat bf16 buffer."""
        from frtm_vos_amd import ops
        B, cin, cout, h, w = self.dims
        ho, wo = self.out_hw
        out = self.out[out_fmt].reset()
        res_fmt = int(res == 'bf16')
        aware = bool(in_fmt or res_fmt or out_fmt)
        c0 = _counts()
        ops.conv2d(self.x[in_fmt].view, self.wT, cout, self.k, self.stride, self.pad, scale=self.sc if scale else None, shift=self.sh if scale else None,
                   residual=None if res is None else self.r[res].view, relu=relu, out=out.view, shape=(B, cin, h, w), w_layout=self.layout, tile=tile,
                   in_fmt=in_fmt, res_fmt=res_fmt, out_fmt=out_fmt)
        names = {t: (n % in_fmt) for t, n in self.names.items()} if aware else self.parents
        assert _last() in names.values() and (tile == 0 or _last() == names[tile]), (_last(), tile, in_fmt, res, out_fmt)
        c1 = _counts()
        moved = tuple(b - a for a, b in zip(c0, c1))
        assert moved == tuple(int(self.layout == l) for l in (L1, S1, S2)) + (int(aware),), moved       # its layout's counter, and the mode's own
        torch.cuda.synchronize()
        for f in [out, self.x[in_fmt]] + ([self.r[res]] if res else []):
            assert f.intact(), 'guard band overwritten'
        got = out.view.clone()
        assert not bool(torch.isnan(got.float()).any()), 'unwritten (sentinel) or NaN outputs'
        return got if out_fmt else got.view(B, cout, ho, wo)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32),
                                                                     b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))


# ---- 1. each kernel against its parent
@pytest.mark.parametrize('kind,dims', [(k, d) for k in KINDS for d in SHAPES[k]], ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_every_format_combination_is_an_exact_function_of_the_parent(kind, dims):
    from frtm_vos_amd import ops
    case = Case(kind, *dims)
    B, cin, cout, h, w = dims
    checked = 0
    per_tile = {}
    for tile, scale, relu in itertools.product((0, 1, 2), (False, True), (False, True)):
        parent = {None: case.run(tile, 0, None, 0, scale, relu), 'f32': case.run(tile, 0, 'f32', 0, scale, relu),
                  'bf16': case.run(tile, 0, 'rounded', 0, scale, relu)}          # parent(x, r.bfloat16().float())
        assert not torch.equal(parent['f32'], parent['bf16']) and not torch.equal(parent[None], parent['f32'])      # (the cases differ)
        fp32_out = {}
        for in_fmt, res in itertools.product((0, 1), (None, 'f32', 'bf16')):
            y = parent[res] if (in_fmt, res) in ((0, None), (0, 'f32')) else case.run(tile, in_fmt, res, 0, scale, relu)
            assert _same_bits(y, parent[res]), (tile, scale, relu, in_fmt, res)
            fp32_out[in_fmt, res] = y
            yb = case.run(tile, in_fmt, res, 1, scale, relu)
            assert _same_bits(yb, ops.act_to_bf16(y)), (tile, scale, relu, in_fmt, res, 'bf16 out')
            assert torch.equal(ops.act_from_bf16(yb, y.shape), y.bfloat16().float())
            per_tile.setdefault((scale, relu, in_fmt, res), []).append(yb)
            checked += 2
    for key, outs in per_tile.items():                      # automatic, form 1, form 2: bit-identical
        assert _same_bits(outs[0], outs[1]) and _same_bits(outs[1], outs[2]), key
    assert checked == 3 * 4 * 12
    # ... and the parent is a convolution, not noise
    ref = F.conv2d(case.x_cpu.bfloat16().double(), case.wt_cpu.bfloat16().double(), stride=case.stride, padding=case.pad)
    got = case.run(0, 1, None, 0, False, False)
    assert float((got.double().cpu() - ref).abs().max()) < 1e-3 * max(1.0, float(ref.abs().max()))


# ---- 2. images do not mix
@pytest.mark.parametrize('tile', (1, 2))
@pytest.mark.parametrize('kind', list(KINDS))
def test_a_nan_in_image_0_leaves_image_1_finite(kind, tile):
    from frtm_vos_amd import ops
    dims = SHAPES[kind][0]
    B, cin, cout, h, w = dims
    clean = Case(kind, *dims, seed=2)
    want = ops.act_from_bf16(clean.run(tile, 1, 'bf16', 1, True, False), (B, cout) + clean.out_hw)          # (no ReLU: fmaxf(NaN, 0) is 0)
    for chan, py, px in ((0, 0, 0), (cin - 1, h - 1, w - 1), (17, 7, 13)):      # corners (the last channel: the K tail) and the interior
        xv = clean.x_cpu.clone()
        xv[0, chan, py, px] = float('nan')
        case = Case(kind, *dims, seed=2, x=xv)
        out = case.out[1].reset()
        ops.conv2d(case.x[1].view, case.wT, cout, case.k, case.stride, case.pad, scale=case.sc, shift=case.sh, residual=case.r['bf16'].view, relu=False,
                   out=out.view, shape=(B, cin, h, w), w_layout=case.layout, tile=tile, in_fmt=1, res_fmt=1, out_fmt=1)
        torch.cuda.synchronize()
        assert out.intact() and _last() == case.names[tile] % 1
        got = ops.act_from_bf16(out.view.clone(), (B, cout) + case.out_hw)
        assert bool(torch.isnan(got[0]).any()), (chan, py, px)
        assert bool(torch.isfinite(got[1]).all()) and torch.equal(got[1], want[1]), (chan, py, px)


# ---- 3. refusals
def _desc(**kw):
    from frtm_vos_amd import _hip as H
    d = dict(B=1, Cin=32, Hin=8, Win=8, Cout=32, ksize=3, stride=1, pad=1, relu=0, out_transposed=0, splitk=0, tile=0, w_layout=S1, ws_elems=0, w_pitch=0)
    d.update(kw)
    return H.ConvDesc(*[d[k] for k, _ in H.ConvDesc._fields_])


@pytest.mark.parametrize('bad', [dict(Cin=36, fmts=(1, 0, 0)), dict(Cout=36, fmts=(0, 0, 1)), dict(Cout=36, fmts=(0, 1, 0)),      # C % 8 != 0
                                 dict(w_layout=0, ksize=1, pad=0, fmts=(1, 0, 0)), dict(w_layout=0, ksize=1, pad=0, fmts=(0, 0, 1)),  # a bf16 format with layout 0
                                 dict(w_layout=1, fmts=(0, 1, 0)), dict(w_layout=5, ksize=1, pad=0, fmts=(1, 0, 0)),
                                 dict(splitk=2, fmts=(1, 0, 0)), dict(out_transposed=1, fmts=(1, 0, 0)),
                                 dict(mis='in', fmts=(1, 0, 0)), dict(mis='res', fmts=(0, 1, 0)), dict(mis='out', fmts=(0, 0, 1)),          # a misaligned pointer
                                 dict(stride=2, fmts=(1, 0, 0)), dict(w_layout=S2, fmts=(0, 0, 1)), dict(w_layout=L1, fmts=(1, 0, 0)),      # the layout's own geometry
                                 dict(w_pitch=32, fmts=(1, 0, 0)), dict(tile=3, fmts=(1, 0, 0)), dict(fmts=(2, 0, 0)), dict(fmts=(0, 0, -1))])
def test_ineligible_calls_are_argument_errors_and_launch_nothing(bad):
    L = _lib()
    x, wB, rs = (torch.zeros(1 << 16, device=DEV) for _ in range(3))
    out = Framed(1 << 14)
    bad = dict(bad)
    fmts, mis = bad.pop('fmts'), bad.pop('mis', None)
    d = _desc(**bad)
    before = _counts()
    rc = L.frtm_conv2d_act(ctypes.byref(d), ctypes.c_void_p(x.data_ptr() + (8 if mis == 'in' else 0)), ctypes.c_void_p(wB.data_ptr()), None, None, None,
                           ctypes.c_void_p(rs.data_ptr() + (8 if mis == 'res' else 0)), ctypes.c_void_p(out.view.data_ptr() + (8 if mis == 'out' else 0)), None,
                           fmts[0], fmts[1], fmts[2], None)
    assert rc == -1, (bad, fmts, rc)
    assert b'frtm_conv2d_act' in L.frtm_last_error(), L.frtm_last_error()
    assert _counts() == before and _last() == ''
    torch.cuda.synchronize()
    assert out.intact() and bool((out.buf == SENT).all())                 # nothing was written


def test_all_fp32_formats_are_frtm_conv2d():
    from frtm_vos_amd import ops
    case = Case('3x3', *SHAPES['3x3'][0])
    c0 = _counts()
    a = case.run(1, 0, 'f32', 0, True, True)
    assert _last() == 'k_conv3x3_bf16x1<2>' and _counts()[3] == c0[3]
    B, cin, cout, h, w = case.dims
    b = ops.conv2d(case.x[0].view.view(B, cin, h, w), case.wT, cout, 3, 1, 1, scale=case.sc, shift=case.sh, residual=case.r['f32'].view.view(a.shape), relu=True,
                   w_layout=S1, tile=1)
    assert torch.equal(a, b)


# ---- 4. the trunk, exactly.  96x160 frames are far below the router table's column counts, so the trunks are created under FRTM_BF16X1_MIN_COLS=0.
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


def _pass(ext, img, **kw):
    a = _counts()
    taps = {k: v.clone() for k, v in ext(img, **kw).items()}
    torch.cuda.synchronize()
    return taps, tuple(y - x for x, y in zip(a, _counts()))


_TRUNKS = {}
ARCH = {'resnet18': 18, 'resnet50': 50}


def _trunk(name):
    """(extractor, frames, {mode: taps}) with one lane; left in fp32."""
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    if name not in _TRUNKS:
        ext = _with_min_cols(lambda: ResnetFeatureExtractor(name, seed=0).to(DEV))
        ext.lanes = 1
        img = torch.randint(0, 256, (4, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(11)).to(DEV)
        taps, launches = {}, {}
        for mode in ('fp32', 'bf16x1_3x3', 'bf16x1_act'):
            ext.precision = mode
            taps[mode], launches[mode] = _pass(ext, img)
        ext.precision = 'fp32'
        _TRUNKS[name] = (ext, img, taps, launches)
    return _TRUNKS[name]


def _walk(ext, h, B, H, W, layer1, rounded):
    """The block walk in Python from the pass's own layer1 tap (the stem's output after the 3x3 stride-2 max pool): every conv through ops.conv2d in fp32 NCHW with the route frtm_backbone_conv_route reports
    and the extractor's own weights (BatchNorm folded by upload()'s two lines); `rounded`: conv indices whose OUTPUT is stored as bf16 -- theirs alone
    goes through t.bfloat16().float().  -> the taps layer2 .. layer5."""
    from frtm_vos_amd import ops
    pairs = ext.resnet.conv_bn_pairs()

    def conv(idx, x, residual=None, relu=True):
        cv, bn = pairs[idx]
        scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).float().contiguous()
        shift = (bn.bias - bn.running_mean * scale).float().contiguous()
        lay, tile, _ = h.route(idx, B, tuple(x.shape[-2:]))
        wgt = cv.weight.data.float().contiguous()
        k = wgt.shape[-1]
        assert lay in (0, L1, S1, S2), (idx, lay)               # (what a bf16x1_3x3 trunk takes under FRTM_BF16X1_MIN_COLS=0)
        if lay == 0:
            wT, ktab, got = ops.pack_weights(wgt, halo=False)
        else:
            wT, ktab, got = ops.pack_weights(wgt, bf16x1=True, stride=cv.stride)
        assert got == lay, (idx, lay, got)
        y = ops.conv2d(x, wT, wgt.shape[0], k, cv.stride, k // 2, ktab=ktab, scale=scale, shift=shift, residual=residual, relu=relu, tile=tile, w_layout=lay)
        return y.bfloat16().float() if idx in rounded else y
    x = layer1                  # the tap is the max pool's output (csrc/backbone.hip: the pool writes the layer1 tap), where the blocks begin
    taps = {}
    for s, stage in enumerate(h.blocks(H, W)):
        for bl in stage:
            assert tuple(x.shape[-2:]) == bl['convs'][0][1]
            idn = conv(bl['ds'][0], x, relu=False) if bl['ds'] else x
            y = x
            for idx, hw in bl['convs'][:-1]:
                y = conv(idx, y)
            x = conv(bl['convs'][-1][0], y, residual=idn)
        taps['layer%d' % (s + 2)] = x
    return taps


@pytest.mark.parametrize('name', ('resnet18', 'resnet50'))
def test_trunk_equals_the_walk_with_the_planned_roundings(name):
    ext, img, taps, launches = _trunk(name)
    B, _, H, W = img.shape
    h = Trunk(ARCH[name], bb=ext._handle)
    try:
        ext.precision = 'bf16x1_3x3'
        assert h.plan(B, H, W) == [(0, 0, 0)] * len(h.shapes())
        # (a) no rounding: the walk is the bf16x1_3x3 trunk -- this pins the walk itself on code that exists without the mode
        plain = _walk(ext, h, B, H, W, taps['bf16x1_3x3']['layer1'], set())
        for k in plain:
            assert torch.equal(plain[k], taps['bf16x1_3x3'][k]), k
        assert launches['bf16x1_3x3'][3] == 0
        # (b) the storage roundings of the plan, and nothing else
        ext.precision = 'bf16x1_act'
        plan = h.plan(B, H, W)
        want, routed, _ = h.expected_plan(B, H, W, True)
        assert plan == want
        for s, stage in enumerate(h.blocks(H, W)):          # not vacuous: per stage a block-internal tensor and a block output are bf16
            assert any(plan[bl['convs'][0][0]][2] for bl in stage) and any(plan[bl['convs'][-1][0]][2] for bl in stage[:-1]), s
        rounded = {i for i, f in enumerate(plan) if f[2]}
        walked = _walk(ext, h, B, H, W, taps['bf16x1_act']['layer1'], rounded)
        for k in walked:
            assert torch.equal(walked[k], taps['bf16x1_act'][k]), k
            assert bool(torch.isfinite(walked[k]).all())
        assert any(not torch.equal(taps['bf16x1_act'][k], taps['bf16x1_3x3'][k]) for k in walked)          # (the residual roundings are visible)
        assert torch.equal(taps['bf16x1_act']['layer1'], taps['fp32']['layer1'])                           # the stem stays fp32
        # the pass launched a format-aware kernel for exactly the convs with a bf16 operand; the per-layout counters are those of bf16x1_3x3
        assert launches['bf16x1_act'][3] == sum(1 for f in plan if any(f)) > 0
        assert launches['bf16x1_act'][:3] == launches['bf16x1_3x3'][:3]
    finally:
        ext.precision = 'fp32'


# ---- 5. the default table on small frames
@pytest.mark.parametrize('name', ('resnet18', 'resnet50'))
def test_default_table_routes_nothing_on_small_frames(name, monkeypatch):
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    monkeypatch.delenv('FRTM_BF16X1_MIN_COLS', raising=False)
    ext = ResnetFeatureExtractor(name, seed=0).to(DEV)
    small = torch.randint(0, 256, (2, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(13)).to(DEV)
    ext.precision = 'bf16x1_3x3'
    a, na = _pass(ext, small)
    ext.precision = 'bf16x1_act'
    b, nb = _pass(ext, small)
    assert na == (0, 0, 0, 0) and nb == (0, 0, 0, 0), (na, nb)            # nothing is routed, so nothing is stored as bf16
    assert all(torch.equal(a[k], b[k]) for k in a)


# ---- 6. lanes, graphs, switching, reload
def test_lanes_switching_and_reload_keep_the_taps():
    ext, img, taps, launches = _trunk('resnet18')
    act, f32 = taps['bf16x1_act'], taps['fp32']
    try:
        ext.precision = 'bf16x1_act'
        ext.lanes = 2
        two, n = _pass(ext, img)
        assert n[3] == 2 * launches['bf16x1_act'][3]                     # every lane runs every format-aware conv of its frames
        two_s1, _ = _pass(ext, img, lane_set=1)
        ext.lanes = 1
        for k in act:
            assert torch.equal(two[k], act[k]) and torch.equal(two_s1[k], act[k]), k
        ext.precision = 'fp32'
        back, n = _pass(ext, img)
        assert n == (0, 0, 0, 0) and all(torch.equal(back[k], f32[k]) for k in f32)
        ext.precision = 'bf16x1_act'
        again, n = _pass(ext, img)
        assert n == launches['bf16x1_act'] and all(torch.equal(again[k], act[k]) for k in act)
        ext.precision = 'bf16x1_3x3'                                      # the flag goes off with the mode
        mid, n = _pass(ext, img)
        assert n[3] == 0 and all(torch.equal(mid[k], taps['bf16x1_3x3'][k]) for k in mid)
        ext.precision = 'bf16x1_act'
        ext.upload()                                                      # frtm_backbone_set_conv with the same weights, under the mode
        re, n = _pass(ext, img)
        assert n == launches['bf16x1_act'] and all(torch.equal(re[k], act[k]) for k in act)
    finally:
        ext.precision = 'fp32'
        ext.lanes = 1


def test_graph_recaptured_on_mode_switch():
    ext, img, taps, launches = _trunk('resnet18')
    ext.lanes = 1
    ext.reuse_outputs, ext.use_graph = True, True
    try:
        for first, second in (('fp32', 'bf16x1_act'), ('bf16x1_3x3', 'bf16x1_act')):         # the second pair changes the storage flag alone
            ext.precision = first
            for _ in range(3):
                out = ext(img)
            torch.cuda.synchronize()
            assert any(e['graph'] is not None for e in ext._out_cache.values())
            assert all(torch.equal(out[k], taps[first][k]) for k in out)
            ext.precision = second
            assert not ext._out_cache
            a = _counts()
            for _ in range(3):
                out = ext(img)
            torch.cuda.synchronize()
            assert any(e['graph'] is not None for e in ext._out_cache.values())
            assert _counts()[3] > a[3]
            assert all(torch.equal(out[k], taps[second][k]) for k in out)
    finally:
        ext.reuse_outputs, ext.use_graph = False, False
        ext.precision = 'fp32'
        ext._out_cache.clear()


# ---- 7. against fp64
def _bf16(t):
    return t.float().bfloat16().double()


def _emulate(ext, h, img_u8, B, H, W, round_ops, rounded):
    """fp64 forward of the trunk on the CPU from the extractor's own parameters (BatchNorm folded as upload() folds it).  round_ops: both operands of every
    conv the trunk routes to a bf16x1 layout rounded to bf16 (to nearest even), as the bf16x1_3x3 mode does; rounded: conv indices whose output is
    stored as bf16 -- the storage roundings of the plan."""
    pairs = ext.resnet.conv_bn_pairs()

    def conv(idx, x, pad=None):
        cv, bn = pairs[idx]
        w = cv.weight.data.double().cpu()
        if round_ops and idx > 0 and h.route(idx, B, tuple(x.shape[-2:]))[0] in (L1, S1, S2):
            x, w = _bf16(x), _bf16(w)
        scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).float()
        shift = (bn.bias - bn.running_mean * scale).float()
        return F.conv2d(x, w, stride=cv.stride, padding=w.shape[-1] // 2) * scale.double().cpu().view(1, -1, 1, 1) + shift.double().cpu().view(1, -1, 1, 1)

    def store(idx, y):
        return _bf16(y) if idx in rounded else y
    x = img_u8.double().cpu() * ext.norm_weight.double().cpu() + ext.norm_bias.double().cpu()
    x = F.max_pool2d(torch.relu(conv(0, x)), 3, 2, 1)
    taps = {'layer1': x}                 # the trunk's layer1 tap is the pool's output
    for s, stage in enumerate(h.blocks(H, W)):
        for bl in stage:
            idn = store(bl['ds'][0], conv(bl['ds'][0], x)) if bl['ds'] else x
            y = x
            for idx, _ in bl['convs'][:-1]:
                y = store(idx, torch.relu(conv(idx, y)))
            last = bl['convs'][-1][0]
            x = store(last, torch.relu(conv(last, y) + idn))
        taps['layer%d' % (s + 2)] = x
    return taps


EMULATION_MARGIN = 1.297          # 1.25 x 1.0375, the largest ratio measured on an MI355X (layer2 .. layer5: 1.0000, 1.0000, 1.0375, 0.9656); never above 2


def test_resnet18_trunk_against_the_emulated_roundings():
    """Per tap: max |HIP bf16x1_act - plain fp64| <= m x max |emulation - plain fp64|, the emulation being the same fp64 forward with both operands of
    every routed conv rounded to bf16 AND the storage roundings of frtm_backbone_act_plan.  The margin m exists because the HIP trunk rounds fp32 values
    where the emulation rounds fp64 ones, so single roundings flip; a wrong layout or epilogue misses by orders of magnitude.  m = the largest ratio
    measured on the GPU x 1.25, never above 2 -- the rule of the parent mode's test.
    Measured on an MI355X: ratios 1.0000 (layer2: 1.0528e-02 / 1.0528e-02), 1.0000 (layer3: 1.4769e-02 / 1.4770e-02), 1.0375 (layer4: 1.2828e-02 /
    1.2365e-02), 0.9656 (layer5: 1.2368e-02 / 1.2809e-02), so m = 1.25 x 1.0375 = 1.297 (EMULATION_MARGIN; recorded in profiles/bf16x1_act_time.txt).
    Printed, not gated: the distance of the taps from bf16x1_3x3 and from the fp32 trunk."""
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    ext = _with_min_cols(lambda: ResnetFeatureExtractor('resnet18', seed=4).to(DEV))
    ext.lanes = 1
    B, H, W = 2, 96, 160
    img = torch.randint(0, 256, (B, 3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    h = Trunk(18, bb=ext._handle)
    f32, _ = _pass(ext, img.to(DEV))
    ext.precision = 'bf16x1_3x3'
    b33, _ = _pass(ext, img.to(DEV))
    ext.precision = 'bf16x1_act'
    hip, n = _pass(ext, img.to(DEV))
    plan = h.plan(B, H, W)
    rounded = {i for i, f in enumerate(plan) if f[2]}
    assert rounded and n[3] == sum(1 for f in plan if any(f))
    plain = _emulate(ext, h, img, B, H, W, False, set())
    emu = _emulate(ext, h, img, B, H, W, True, rounded)
    assert 1.0 <= EMULATION_MARGIN <= 2.0
    for k in ('layer2', 'layer3', 'layer4', 'layer5'):
        d_hip = float((hip[k].double().cpu() - plain[k]).abs().max())
        d_emu = float((emu[k] - plain[k]).abs().max())
        d_f32 = float((f32[k].double().cpu() - plain[k]).abs().max())
        rng = float(plain[k].abs().max())
        print('resnet18 %s: max|HIP - plain| %.4e, max|emulation - plain| %.4e, ratio %.4f (m = %.3f); max|HIP - emulation| %.3e; fp32 trunk - plain %.3e; '
              'bf16x1_act - bf16x1_3x3 %.3e, bf16x1_act - fp32 trunk %.3e, of max|plain| %.3e' % (
                  k, d_hip, d_emu, d_hip / d_emu, EMULATION_MARGIN, float((hip[k].double().cpu() - emu[k]).abs().max()), d_f32,
                  float((hip[k] - b33[k]).abs().max()), float((hip[k] - f32[k]).abs().max()), rng))
        assert d_emu > 100 * d_f32, k
        assert d_hip <= EMULATION_MARGIN * d_emu, (k, d_hip, d_emu)
    assert torch.equal(hip['layer1'], f32['layer1'])


def test_trunk_vs_oracle_is_printed_not_gated():
    """Taps of the bf16x1_act trunk against the CPU oracle next to those of bf16x1_3x3 and the fp32 trunk: printed.  No numeric gate: the figure cannot be
    derived, and it must not be set from the code under test."""
    from oracle import cpu_ref as O
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    torch.set_grad_enabled(False)
    name = 'resnet18'
    P = O.resnet_random_params(name, seed=3)
    img = torch.randint(0, 256, (4, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    ref = O.resnet_forward(name, P, img)
    ext = _with_min_cols(lambda: ResnetFeatureExtractor(name, weights=P).to(DEV))
    ext.lanes = 1
    out = {}
    for mode in ('fp32', 'bf16x1_3x3', 'bf16x1_act'):
        ext.precision = mode
        out[mode], n = _pass(ext, img.to(DEV))
        assert (n[3] > 0) == (mode == 'bf16x1_act'), (mode, n)
    for k in sorted(ref):
        e = [float((out[m][k].double().cpu() - ref[k].double()).abs().max() / (ref[k].double().abs().max() + 1e-30)) for m in ('fp32', 'bf16x1_3x3', 'bf16x1_act')]
        print('%s B=4 %s: rel err against the oracle fp32 %.3e bf16x1_3x3 %.3e bf16x1_act %.3e' % (name, k, e[0], e[1], e[2]))
        assert bool(torch.isfinite(out['bf16x1_act'][k]).all()), k


# ---- 8. tracker plumbing
def test_tracker_runs_with_a_bf16x1_act_resnet18_trunk():
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    torch.set_grad_enabled(False)
    seq = SyntheticSequence('bf16x1_act', 4, (96, 160), 2, seed=31)
    seq.preload(DEV)
    torch.manual_seed(0)
    params = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18', trunk_precision='bf16x1_act')
    trk = _with_min_cols(lambda: params.get_model().eval())          # every eligible conv of the trunk is routed
    assert trk.feature_extractor.precision == 'bf16x1_act'
    a = _counts()
    image, lb, new_objects = seq[0]
    masks = trk.initialize(image.to(DEV), lb.to(DEV), new_objects)
    assert bool(torch.isfinite(masks).all())
    for t in range(1, 4):
        trk.current_frame += 1
        masks = trk.track(seq[t][0].to(DEV))
        assert tuple(masks.shape) == (3, 96, 160) and bool(torch.isfinite(masks).all()), t
    torch.cuda.synchronize()
    b = _counts()
    assert b[3] > a[3] and b[1] > a[1] and b[2] > a[2] and b[0] == a[0]          # format-aware launches of both 3x3 layouts; ResNet-18 has no 1x1 conv to route
