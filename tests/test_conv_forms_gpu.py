"""Every compiled convolution kernel form (tests/test_conv_forms.py: FORMS) against an exact reference, at the shapes where tiled kernels go wrong.

Inputs are small integers (x, w in -2..2), BN scale a power of two, BN shift and residual multiples of 1/4: every product and partial sum is an integer
below 2^24, so an fp32 accumulation is exact in any order and every direct / implicit-GEMM form -- and the fused Winograd F(2x2,3x3) kernel, whose
transforms only add, subtract and halve -- must equal an fp64 convolution BIT FOR BIT.  The F(4x4,3x3) / F(6x6,3x3) three-launch forms (transforms not
exact in binary) run on random-normal data against an element-wise bound |out - ref| <= tau * A, A = |scale| conv(|x|, |w|) + |shift| + |res|.

Every call writes into an output filled with NaN and framed by sentinel words (the split-K workspace as well); the input and the residual are framed by
NaN.  After each call: the sentinels are intact, no NaN is left, the values are exact.  frtm_conv_last_kernels() names the kernels each call launched;
each case asserts the form it meant to reach, and the last test asserts that the module reached every listed form."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from test_conv_forms import EXCEPTIONS, FORMS

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1500)]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda'
GUARD = 256                   # floats of guard band on each side (a multiple of 4: the framed tensors keep 16-byte alignment)
SENT = 0x7FA5A5A5             # sentinel word (a NaN pattern no kernel produces)
SEEN = set()                  # kernel names reached by this module
CASES_RUN = []

# element-wise bounds of the three-launch Winograd forms: measured worst |out - ref| / A over the cases below 2.4e-6 (F4) and 4.9e-6 (F6) on MI355X, about 4x margin
TAU = {4: 1e-5, 6: 2e-5}

T64, T32, T128, T64W8, T64x128, T128x128, T128x128W16, T80, TG32 = 1, 2, 3, 4, 7, 8, 9, 10, 23
TILE = {T64: (64, 64, 2, 2), T32: (32, 64, 1, 4), T128: (128, 64, 2, 2), T64W8: (64, 64, 2, 4), T64x128: (64, 128, 2, 4),
        T128x128: (128, 128, 2, 4), T128x128W16: (128, 128, 4, 4)}
HALO_TILE = {32: (T32, 1, 4), 64: (T64, 2, 2), 80: (T80, 1, 4), 128: (T128, 2, 2)}


def _lib():
    from frtm_vos_amd import _hip as H
    return H.lib()


def _last_kernels():
    names = _lib().frtm_conv_last_kernels().decode().split()
    SEEN.update(names)
    return names


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


def _ints(g, *shape):
    return torch.randint(-2, 3, shape, generator=g).float()


def _epilogue(g, cout, B, Ho, Wo):
    scale = (2.0 ** torch.randint(-2, 3, (cout,), generator=g)) * (torch.randint(0, 2, (cout,), generator=g) * 2 - 1)
    shift = torch.randint(-12, 13, (cout,), generator=g) / 4.0
    res = torch.randint(-12, 13, (B, cout, Ho, Wo), generator=g) / 4.0
    return scale.float(), shift.float(), res.float()


def _reference(x, w, stride, pad, epi, relu):
    ref = F.conv2d(x.double(), w.double(), stride=stride, padding=pad)
    if epi is not None:
        scale, shift, res = epi
        ref = ref * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1) + res.double()
    if relu:
        ref = torch.relu(ref)
    return ref


def conv_case(B, cin, cout, h, w, k=3, stride=1, layout='gemm', tile=0, splitk=1, epi=False, transposed=False, ws_elems=None, seed=0,
              exact=True, expect=None, data=None):
    """One frtm_conv2d call on framed, poisoned buffers.  Returns (kernel names, out as float64 CPU, fp64 reference, A)."""
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(seed * 7919 + B * 1009 + cin * 101 + cout * 11 + h + w)
    pad = k // 2
    Ho, Wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    if data is None:
        x, wt = _ints(g, B, cin, h, w), _ints(g, cout, cin, k, k)
    else:
        x, wt = data(g, (B, cin, h, w), (cout, cin, k, k))
    ep = _epilogue(g, cout, B, Ho, Wo) if epi else None
    relu = epi
    wT, ktab, lay = ops.pack_weights(wt.to(DEV), halo=(layout == 'halo'), wino=(layout == 'wino'), wino4=(layout == 'wino4'), wino6=(layout == 'wino6'))
    pack = _last_kernels()
    assert pack == [{'gemm': 'k_pack_weights', 'halo': 'k_pack_weights_halo', 'wino': 'k_pack_weights_wino', 'wino4': 'k_wino4_weights',
                     'wino6': 'k_wino6_weights'}[layout]], pack
    xin = _nan_framed(x)
    sc = sh = rs = None
    if epi:
        sc, sh, rs = ep[0].to(DEV), ep[1].to(DEV), _nan_framed(ep[2])
    out_elems = B * cout * Ho * Wo
    out = Framed(out_elems)
    out.view.fill_(float('nan'))
    ws = None
    if layout in ('wino4', 'wino6'):
        m = 4 if layout == 'wino4' else 6
        tiles = (B * ((h + m - 1) // m) * ((w + m - 1) // m) + 63) // 64 * 64
        ws = Framed((m + 2) ** 2 * (cin + cout) * tiles if ws_elems is None else ws_elems)
    elif splitk != 1:
        ws = Framed(ws_elems if ws_elems is not None else min(32 * out_elems, max(2 * out_elems, 1 << 24)))
    oshape = (B, Ho * Wo, cout) if transposed else (B, cout, Ho, Wo)
    ops.conv2d(xin, wT, cout, k, stride, pad, ktab=ktab, scale=sc, shift=sh, residual=rs, relu=relu, out=out.view.view(oshape),
               out_transposed=transposed, splitk=splitk, tile=tile, w_layout=lay, ws=None if ws is None else ws.view)
    names = _last_kernels()
    torch.cuda.synchronize()
    CASES_RUN.append(names)
    label = (B, cin, cout, h, w, k, stride, layout, tile, splitk, epi, transposed, names)
    if expect is not None:
        assert names == expect, label
    assert out.intact(), ('output guard band overwritten',) + label
    if ws is not None:
        assert ws.intact(), ('workspace guard band overwritten',) + label
    got = out.view.view(oshape).cpu()
    if transposed:
        got = got.permute(0, 2, 1).reshape(B, cout, Ho, Wo)
    assert not torch.isnan(got).any(), ('unwritten (NaN) outputs: %d' % int(torch.isnan(got).sum()),) + label
    ref = _reference(x, wt, stride, pad, ep, relu)
    if exact:
        bad = got.double() != ref
        assert not bad.any(), ('%d of %d outputs differ from the exact value, max |err| %g' % (int(bad.sum()), bad.numel(),
                                                                                            float((got.double() - ref).abs().max())),) + label
        return names, got.double(), ref, None
    A = F.conv2d(x.double().abs(), wt.double().abs(), stride=stride, padding=pad)
    if epi:
        A = A * ep[0].double().abs().view(1, -1, 1, 1) + ep[1].double().abs().view(1, -1, 1, 1) + ep[2].double().abs()
    return names, got.double(), ref, A


def _igemm(tile, mode):
    return 'k_conv_igemm<%d,%d,%d,%d,%d,32>' % (TILE[tile] + (mode,))


# ---- implicit-GEMM tiles, MODE 0 (gather: 3x3 / 7x7 with ktab, strided 1x1) ----
@pytest.mark.parametrize('tile', sorted(TILE))
@pytest.mark.parametrize('B,cin,cout,h,w,k,stride,epi', [
    (2, 5, 33, 11, 11, 3, 1, False),         # K = 45: a K tail; Cout 33; 242 columns: ragged, tiles straddle the two images
    (3, 7, 81, 13, 17, 3, 2, True),          # stride 2 on odd sizes, Cout 81, epilogue
    (2, 40, 129, 9, 11, 1, 2, True),         # strided 1x1 (the downsample form), Cout 129
    (1, 3, 65, 21, 15, 7, 2, False),         # 7x7 stride 2 (the stem form), K = 147
    (1, 9, 33, 1, 1, 3, 1, True),            # a 1x1 map: every tap but the centre is padding
])
def test_igemm_gather_forms(tile, B, cin, cout, h, w, k, stride, epi):
    conv_case(B, cin, cout, h, w, k, stride, tile=tile, splitk=1, epi=epi, expect=[_igemm(tile, 0)])


# ---- MODE 1 (stride-1 1x1, H*W % 4 == 0: dwordx4 staging) ----
@pytest.mark.parametrize('tile', sorted(TILE))
@pytest.mark.parametrize('B,cin,cout,h,w,epi', [
    (2, 37, 65, 6, 10, True),                # K tail, Cout 65, 120 columns: a tile straddles the two images
    (3, 64, 128, 8, 12, False),              # 288 columns: Ntot % 128 != 0
    (1, 32, 33, 2, 2, True),                 # 4 pixels
])
def test_igemm_vec_forms(tile, B, cin, cout, h, w, epi):
    conv_case(B, cin, cout, h, w, 1, 1, tile=tile, splitk=1, epi=epi, expect=[_igemm(tile, 1)])


# ---- MODE 2 (stride-1 1x1, H*W % 4 != 0) ----
@pytest.mark.parametrize('tile', [T64, T32, T64W8])
@pytest.mark.parametrize('B,cin,cout,h,w,epi', [
    (3, 33, 80, 5, 7, True),                 # 35 pixels: lanes whose four columns straddle an image end
    (2, 64, 64, 3, 9, False),
    (4, 8, 33, 1, 5, True),                  # 5 pixels per image, 20 columns
])
def test_igemm_unaligned_forms(tile, B, cin, cout, h, w, epi):
    conv_case(B, cin, cout, h, w, 1, 1, tile=tile, splitk=1, epi=epi, expect=[_igemm(tile, 2)])


# ---- G32 (1x1, stride 1, 16-byte aligned) ----
@pytest.mark.parametrize('B,cin,cout,h,w,epi', [(2, 40, 65, 6, 10, True), (1, 64, 128, 8, 8, False), (3, 96, 33, 5, 12, True)])
def test_g32_form(B, cin, cout, h, w, epi):
    conv_case(B, cin, cout, h, w, 1, 1, tile=TG32, splitk=1, epi=epi, expect=['k_conv1x1_g32<1,1,2,2,0,2>'])


# ---- 3x3 halo kernels: every BM x TW x stride.  The tile width is the library's choice (halo_tile_width: fewest padded tiles, ties to 8, 16, 4);
# the output sizes below make each width win: 31x3 -> 4, 15x15 -> 8, 3x37 -> 16.  Cin 11: a tail chunk of 3 channels (HCI = 8).
HALO_OUT = {4: (31, 3), 8: (15, 15), 16: (3, 37)}


@pytest.mark.parametrize('bm', sorted(HALO_TILE))
@pytest.mark.parametrize('tw', [4, 8, 16])
@pytest.mark.parametrize('stride', [1, 2])
@pytest.mark.parametrize('epi', [False, True])
def test_halo_forms(bm, tw, stride, epi):
    tile, wgm, wgn = HALO_TILE[bm]
    Ho, Wo = HALO_OUT[tw]
    h, w = (Ho, Wo) if stride == 1 else (2 * Ho - 1, 2 * Wo - 1)           # stride 2: odd input sizes
    B, cout = (2, bm + 1) if not epi else (1, bm // 2 + 1)                   # Cout just past one tile / below one tile
    conv_case(B, 11, cout, h, w, 3, stride, layout='halo', tile=tile, splitk=1, epi=epi,
              expect=['k_conv3x3_halo<%d,%d,%d,%d,%d>' % (bm, wgm, wgn, tw, stride)])


@pytest.mark.parametrize('bm', sorted(HALO_TILE))
@pytest.mark.parametrize('stride', [1, 2])
def test_halo_tiny_maps(bm, stride):
    """A 1x1 output (Wo < TW; every tap but one is padding) and a 2x5 output, B = 3."""
    tile, wgm, wgn = HALO_TILE[bm]
    for (h, w) in ((1, 1), (2 * stride - 1 if stride == 2 else 2, 9 if stride == 2 else 5)):
        Ho, Wo = (h - 1) // stride + 1, (w - 1) // stride + 1
        tw = min((8, 16, 4), key=lambda t: ((Ho + 64 // t - 1) // (64 // t)) * ((Wo + t - 1) // t))
        conv_case(3, 16, bm - 3, h, w, 3, stride, layout='halo', tile=tile, splitk=1, epi=True,
                  expect=['k_conv3x3_halo<%d,%d,%d,%d,%d>' % (bm, wgm, wgn, tw, stride)])


# ---- split-K (k_splitk_epilogue), the workspace clamp, out_transposed ----
@pytest.mark.parametrize('splitk', [2, 3, 32])
def test_splitk_gemm(splitk):
    # 1x1 stride 2, K = 1024: 32 chunks, so a split of 32 is 32 slabs
    conv_case(1, 1024, 65, 9, 9, 1, 2, tile=T64, splitk=splitk, epi=True, expect=[_igemm(T64, 0), 'k_splitk_epilogue'])
    # 3x3, K = 1152 = 36 chunks (3 -> 12 per slab; 32 -> 2 per slab, 18 slabs)
    conv_case(2, 128, 33, 7, 5, 3, 1, tile=T32, splitk=splitk, epi=False, expect=[_igemm(T32, 0), 'k_splitk_epilogue'])
    # MODE 1 and MODE 2 launches with split-K
    conv_case(2, 256, 64, 4, 6, 1, 1, tile=T64W8, splitk=splitk, epi=True, expect=[_igemm(T64W8, 1), 'k_splitk_epilogue'])
    conv_case(2, 256, 64, 3, 5, 1, 1, tile=T32, splitk=splitk, epi=True, expect=['k_conv_igemm<32,64,1,4,2,32>', 'k_splitk_epilogue'])


@pytest.mark.parametrize('splitk', [2, 3, 32])
def test_splitk_halo(splitk):
    # Cin 256: 32 chunks of 8 channels
    conv_case(2, 256, 33, 9, 11, 3, 2, layout='halo', tile=T64, splitk=splitk, epi=True, expect=['k_conv3x3_halo<64,2,2,8,2>', 'k_splitk_epilogue'])
    conv_case(1, 250, 81, 4, 13, 3, 1, layout='halo', tile=T80, splitk=splitk, epi=False, expect=['k_conv3x3_halo<80,1,4,16,1>', 'k_splitk_epilogue'])


def test_splitk_workspace_clamp():
    """A workspace that holds two partial slabs (plus a few words): the library must cut a requested split of 8 to 2 -- a third slab would land in
    the guard band."""
    for layout, tile, k, expect in (('gemm', T64, 3, _igemm(T64, 0)), ('halo', T32, 3, 'k_conv3x3_halo<32,1,4,8,1>')):
        B, cout, h, w = 2, 40, 7, 9
        conv_case(B, 128, cout, h, w, k, 1, layout=layout, tile=tile, splitk=8, epi=True, ws_elems=2 * B * cout * h * w + 7,
                  expect=[expect, 'k_splitk_epilogue'])
        # room for less than two slabs: no split at all
        conv_case(B, 128, cout, h, w, k, 1, layout=layout, tile=tile, splitk=8, epi=True, ws_elems=2 * B * cout * h * w - 1, expect=[expect])


@pytest.mark.parametrize('splitk', [1, 3])
def test_out_transposed(splitk):
    tail = ['k_splitk_epilogue'] if splitk > 1 else []
    conv_case(2, 20, 33, 9, 9, 3, 1, tile=T32, splitk=splitk, epi=True, transposed=True, expect=[_igemm(T32, 0)] + tail)
    conv_case(2, 64, 65, 6, 10, 1, 1, tile=T64, splitk=splitk, epi=False, transposed=True, expect=[_igemm(T64, 1)] + tail)
    conv_case(3, 64, 65, 3, 5, 1, 1, tile=T64W8, splitk=splitk, epi=True, transposed=True, expect=[_igemm(T64W8, 2)] + tail)
    conv_case(2, 24, 33, 15, 15, 3, 1, layout='halo', tile=T32, splitk=splitk, epi=True, transposed=True,
              expect=['k_conv3x3_halo<32,1,4,8,1>'] + tail)


# ---- fused Winograd F(2x2,3x3): exact on integer data (the transforms only add, subtract and halve) ----
@pytest.mark.parametrize('variant,name', [(1, 'k_conv3x3_wino<1,0,5>'), (2, 'k_conv3x3_wino<2,0,3>'), (3, 'k_conv3x3_wino<2,1,3>')])
@pytest.mark.parametrize('B,cin,cout,h,w,epi', [
    (2, 11, 33, 13, 19, False),              # Cin tail, Cout 33, maps no multiple of the 8x8 / 8x16 / 16x8 block, odd sizes
    (1, 16, 64, 17, 9, True),
    (3, 8, 20, 1, 1, True),                  # a 1x1 map
    (1, 24, 40, 2, 3, False),
])
def test_winograd_f2_forms(variant, name, B, cin, cout, h, w, epi):
    conv_case(B, cin, cout, h, w, 3, 1, layout='wino', tile=variant, epi=epi, expect=[name])


# ---- three-launch Winograd F(4x4,3x3) / F(6x6,3x3): random-normal data, element-wise bound ----
def _normal(g, xs, ws):
    x = torch.relu(torch.randn(*xs, generator=g))
    return x, torch.randn(*ws, generator=g) / (9 * ws[1]) ** 0.5


@pytest.mark.parametrize('m', [4, 6])
def test_winograd_three_launch_forms(m):
    worst = 0.0
    for (B, cin, cout, h, w, tile, epi) in [(3, 128, 64, 30, 54, 0, True), (2, 160, 128, 17, 23, T64, False), (1, 40, 33, 7, 11, T32, True),
                                            (2, 96, 192, 9, 13, T64W8, True)]:
        for seed in (0, 1):
            names, got, ref, A = conv_case(B, cin, cout, h, w, 3, 1, layout='wino%d' % m, tile=tile, epi=epi, exact=False, data=_normal, seed=seed)
            assert names[0] == 'k_wino%d_input' % m and names[-1] == 'k_wino%d_output' % m and len(names) == 3, names
            err = (got - ref).abs()
            ratio = float((err / A.clamp_min(1e-30)).max())
            worst = max(worst, ratio)
            assert ratio <= TAU[m], (m, B, cin, cout, h, w, tile, epi, ratio)
            assert float(err.max() / ref.abs().max()) < 3e-5                 # the gate of tests/test_round3_gpu.py, kept
    print('\nF(%dx%d,3x3): worst |out - ref| / A = %.3e (tau %.1e)' % (m, m, worst, TAU[m]))


# ---- the real 480x854 trunk (ResNet-101) and refiner shapes, the planner's own tile and split-K (as backbone.hip / seg_network.py launch them:
# 3x3 convs on the halo layout, the rest on the GEMM layout, a workspace the size the backbone gives) ----
TRUNK = [
    # (name, cin, cout, h, w, k, stride, layout, expected first kernel or None)
    ('stem', 3, 64, 480, 854, 7, 2, 'gemm', None),
    ('layer1 1x1 64->256', 64, 256, 120, 214, 1, 1, 'gemm', None),
    ('layer1 3x3', 64, 64, 120, 214, 3, 1, 'halo', None),
    ('layer2 3x3 stride 2', 128, 128, 120, 214, 3, 2, 'halo', 'k_conv3x3_halo<64,2,2,16,2>'),
    ('layer2 downsample', 256, 512, 120, 214, 1, 2, 'gemm', None),
    ('layer3 3x3 stride 2', 256, 256, 60, 107, 3, 2, 'halo', 'k_conv3x3_halo<64,2,2,8,2>'),
    ('layer3 1x1 1024->256', 1024, 256, 30, 54, 1, 1, 'gemm', None),
    ('layer4 3x3 stride 2', 512, 512, 30, 54, 3, 2, 'halo', 'k_conv3x3_halo<64,2,2,4,2>'),
    ('layer4 1x1 2048->512', 2048, 512, 15, 27, 1, 1, 'gemm', None),
    ('refiner TSE 3x3 ->65', 64, 65, 60, 107, 3, 1, 'halo', 'k_conv3x3_halo<80,1,4,16,1>'),
    ('refiner 1x1 96->64', 96, 64, 30, 54, 1, 1, 'gemm', None),
]


@pytest.mark.parametrize('B', [1, 8])
@pytest.mark.parametrize('name,cin,cout,h,w,k,stride,layout,first', TRUNK, ids=[t[0] for t in TRUNK])
def test_trunk_shapes_under_the_planner(B, name, cin, cout, h, w, k, stride, layout, first):
    Ho, Wo = (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1
    out_elems = B * cout * Ho * Wo
    names = conv_case(B, cin, cout, h, w, k, stride, layout=layout, tile=0, splitk=0, epi=True,
                      ws_elems=max(min(32 * out_elems, 16 << 20), 2 * out_elems))[0]
    if first is not None:
        assert names[0] == first, (name, B, names)
    assert names[1:] in ([], ['k_splitk_epilogue']), names


# ---- the persistent GEMM (k_conv_igemm_p), in a fresh process: its grid and gate are read once per process ----
PERSIST_CASES = [
    # (B, cin, cout, h, w, residual): G = 256 workgroups (one per CU), FRTM_PERSIST_MIN_ROUNDS_X2 = 1 (the form from G / 2 tiles on)
    (2, 64, 64, 78, 82, True),      # 200 tiles < G: 56 surplus workgroups; the last tile of each image straddles into the next
    (1, 64, 128, 78, 82, False),    # 200 tiles, Mt = 2
    (2, 64, 192, 50, 82, True),     # 387 tiles: just above 1.5 G, 387 % 8 != 0, K = 64 (one chunk pair)
    (4, 128, 256, 50, 82, False),   # 1028 tiles: five rounds
]


def _persistent_child():
    """Runs in the child: every case through the persistent form and through the plain 64x64 kernel; prints one JSON line."""
    from frtm_vos_amd import ops
    import ctypes
    info = (ctypes.c_int * 4)()
    assert _lib().frtm_device_info(info) == 0
    G = info[0] // 8 * 8
    report = {'G': G, 'cases': []}
    for (B, cin, cout, h, w, res) in PERSIST_CASES:
        ntiles = (cout // 64) * ((B * h * w + 63) // 64)
        n0 = _lib().frtm_conv_persistent_launches()
        names, got, ref, _ = conv_case(B, cin, cout, h, w, 1, 1, tile=T64W8, splitk=1, epi=res, expect=['k_conv_igemm_p'])
        assert _lib().frtm_conv_persistent_launches() == n0 + 1
        plain = conv_case(B, cin, cout, h, w, 1, 1, tile=T64, splitk=1, epi=res, expect=[_igemm(T64, 1)])[1]
        assert torch.equal(got, plain)
        report['cases'].append([B, cin, cout, h, w, res, ntiles])
    report['seen'] = sorted(SEEN)
    print('PERSIST ' + json.dumps(report))


def test_persistent_form_with_surplus_workgroups():
    """k_conv_igemm_p with more workgroups than tiles (FRTM_PERSIST_MIN_ROUNDS_X2 = 1, one workgroup per CU): the surplus workgroups must not touch
    the output -- exact values, guard bands intact, no NaN left -- and the tile walk must cover every tile at the 1.5 x G gate and over several rounds.
    (Before the kernel returned early for them, surplus workgroups recomputed tiles of other workgroups and stored the same values again, or stored
    past the output where the buffer descriptor drops the writes: wasted work and racing stores rather than wrong values, which is why this test also
    passes without that return.)"""
    env = dict(os.environ, FRTM_PERSIST_MIN_ROUNDS_X2='1', FRTM_PERSIST_WG_PER_CU='1', PYTHONPATH=ROOT)
    env.pop('FRTM_NO_PERSIST_GEMM', None)
    p = subprocess.run([sys.executable, '-s', os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('PERSIST ')]
    assert line, p.stdout[-3000:]
    rep = json.loads(line[-1][len('PERSIST '):])
    G = rep['G']
    tiles = [c[-1] for c in rep['cases']]
    assert any(G // 2 <= t < G for t in tiles), (G, tiles)                   # surplus workgroups were launched
    assert any(1.5 * G < t < 1.6 * G and t % 8 for t in tiles), (G, tiles)
    SEEN.update(rep['seen'])
    CASES_RUN.append(rep['seen'])


def test_every_listed_form_was_reached():
    """Runs last: the kernels named by the calls above are exactly the listed forms (EXCEPTIONS cannot be launched through the C ABI)."""
    if len(CASES_RUN) < 200:
        pytest.skip('only part of the module ran (%d calls)' % len(CASES_RUN))
    assert FORMS - SEEN == set(), sorted(FORMS - SEEN)
    assert SEEN - FORMS == set(), sorted(SEEN - FORMS)
    assert not SEEN & set(EXCEPTIONS)


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    _persistent_child()
