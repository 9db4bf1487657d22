"""tests/_image_refs.py pinned without a GPU: each definition equals the oracle's where the oracle has one (exactly, in float64), the
exact-transform set has the properties tests/test_image_ops_gpu.py relies on, no envelope of a quantised output is vacuous, and every
kernel of csrc/image_ops.hip has a GPU test that launches it."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _image_refs as R
from oracle import aug_ref, warp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------------------------
# completeness
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_kernel_of_image_ops_has_a_gpu_test():
    src = open(os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'image_ops.hip')).read()
    kernels = set(re.findall(r'__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?void\s+(\w+)\s*\(', src))
    assert len(kernels) == src.count('__global__') >= 12, sorted(kernels)          # the expression found every kernel of the file
    assert kernels - set(R.KERNELS) == set(), 'kernels no test reaches: add cases to tests/test_image_ops_gpu.py and list them in _image_refs.KERNELS'
    assert set(R.KERNELS) - kernels == set(), 'listed kernels that no longer exist'
    gpu = open(os.path.join(ROOT, 'tests', 'test_image_ops_gpu.py')).read()
    defined = set(re.findall(r'^def (test_\w+)\(', gpu, flags=re.M))
    for k, tests in R.KERNELS.items():
        assert tests and set(tests) <= defined, (k, set(tests) - defined)
    # every launcher of the file is called by name in the GPU module (a kernel is reached through its entry point)
    for entry in re.findall(r'extern "C" int (frtm_\w+)\(', src):
        assert ("'%s'" % entry) in gpu or (entry == 'frtm_fill32' and 'H.fill(' in gpu), entry


# ---------------------------------------------------------------------------------------------------------------------------------
# the definitions against the oracle's, exact in float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Hh,Ww,pattern', [c for c in R.PP_CASES if c[0] <= 100])
def test_pull_push_equals_the_oracle(Hh, Ww, pattern):
    for integer in (False, True):
        level0 = R.pull_push_level0(Hh, Ww, pattern, integer)
        levels, q = R.pull_push_fill(level0, F64)
        image = R.pull_push_image(Hh, Ww, integer)                  # the image level 0 was cut from, hole pixels included
        assert torch.equal(image * level0[3:], level0[:3]) and bool((image == image.floor()).all()) == integer
        want = aug_ref.pull_push_fill_ref(image, 1 - level0[3:], F64)
        assert torch.equal(q, want)
    assert [tuple(l.shape[-2:]) for l in levels] == R.pull_push_sizes(Hh, Ww)
    assert sum(l.numel() for l in levels) == R.pull_push_elems(Hh, Ww)
    assert torch.equal(levels[0][:3].clamp(0, 255).floor(), q) and torch.equal(levels[0][3:], level0[3:].double())
    known = level0[3] > 0
    assert torch.equal(q[:, known], level0[:3, known].double())                               # known pixels keep their (integer) values
    if pattern == 'nothing_known':
        assert float(q.abs().max()) == 0.0 and all(float(l.abs().max()) == 0.0 for l in levels)
    if (Hh, Ww) == (2, 7):
        assert len(levels) == 1
    if (Hh, Ww) == (100, 3):
        assert len(levels) == 2


def test_pull_push_sizes():
    assert R.pull_push_sizes(1030, 1030)[1:4] == [(515, 515), (258, 258), (129, 129)] and R.pull_push_sizes(1030, 1030)[-1] == (2, 2)
    assert R.pull_push_sizes(37, 53) == [(37, 53), (19, 27), (10, 14), (5, 7), (3, 4), (2, 2)]       # odd at different levels in H and W
    assert R.pull_push_sizes(65, 129) == [(65, 129), (33, 65), (17, 33), (9, 17), (5, 9), (3, 5), (2, 3)]
    assert 4 * R.PP_LARGE[0] * R.PP_LARGE[1] > 4 * 2048 * 256 and 515 * 515 > 1024 * 256                # both grid-stride loops take a second trip
    assert len(R.pull_push_sizes(5000, 5000)) == 11


@pytest.mark.parametrize('half', R.BLUR_HALVES)
def test_blur_definitions(half):
    for qi, (qa, qb, qc) in enumerate(R.BLUR_Q):
        x = torch.randn(2, 15, 17, generator=R.gen(half, qi), dtype=F64) * 50
        want = aug_ref.gauss_blur_ref(x, ('gauss', half, qa, qb, qc), F64)
        assert torch.equal(R.blur_gauss2d(x, half, qa, qb, qc, F64), want)
        # the tap form sums the same products in another order: agreement to rounding of the sum, 1e-13 of its magnitude
        taps = R.blur_gauss2d(x, half, qa, qb, qc, F64, taps=True)
        assert float((taps - want).abs().max()) <= 1e-13 * float(x.abs().max())
        g = R.gauss_table(half, qa, qb, qc)
        assert abs(float(g.sum()) - 1) < 1e-14 and g.shape == (2 * half + 1, 2 * half + 1)
    G = torch.randn(9, 3, generator=R.gen(half, 5), dtype=F64)
    x = torch.randn(3, 15, 17, generator=R.gen(half, 6), dtype=F64)
    want = F.conv2d(x[:, None], G[None, None], padding=(4, 1))[:, 0]
    assert float((R.blur2d(x, G, F64) - want).abs().max()) <= 1e-13 * float(x.abs().max() * G.abs().sum())


def test_blur_spec_is_the_products():
    from frtm_vos_amd.model.augmenter import ImageAugmenter
    for bs in (1.0, 2.0, 5.0):
        for ang in (0, 45, 90, 135):
            assert ('gauss',) + R.blur_spec(bs, ang) == ImageAugmenter._blur_spec(dict(blur_size=bs, blur_angle=ang))
    assert sorted({R.blur_spec(bs, 0)[0] for bs in (1.0, 2.0, 5.0)}) == [1, 3]


def _general_transforms(Hs, Ws):
    return [('general%d' % k, T[:2].ravel()) for k, T in enumerate(warp_ref.augmenter_like_transforms((Hs, Ws), n=3, seed=5))]


@pytest.mark.parametrize('sizes', R.WARP_SIZES, ids=str)
def test_warp_equals_the_oracle(sizes):
    (Hs, Ws), (Hd, Wd) = sizes
    for C in (1, 3):
        for u8 in (False, True):
            for name, fwd in R.exact_transforms(Hs, Ws, Hd, Wd) + _general_transforms(Hs, Ws):
                inv = warp_ref.inverse_affine(fwd.reshape(2, 3)).ravel()
                for mode in R.MODES:
                    src = R.warp_source_u8(C, Hs, Ws, mode) if u8 else R.warp_source_f32(C, Hs, Ws)
                    v = R.warp_affine(src, inv, (Hd, Wd), mode, F64)
                    want = warp_ref.warp_affine_ref(src, fwd.reshape(2, 3), (Hd, Wd), mode, F64)
                    got = R.round_u8(v) if src.dtype == torch.uint8 else v
                    assert got.dtype == want.dtype and torch.equal(got, want), (name, mode, C)
                    if name == 'nothing_inside':
                        assert float(v.abs().max()) == 0.0


def test_paste_and_label_lines_equal_augment_ref():
    """augment_ref's whole composition from these definitions: prepare, fill, bicubic warps clamped, blur, paste, label."""
    Hh, Ww = 37, 53
    g = R.gen(37, 53, 1)
    image = torch.randint(0, 256, (3, Hh, Ww), generator=g).to(torch.uint8)
    label = torch.zeros(Hh, Ww, dtype=torch.uint8)
    label[10:25, 20:41] = 2
    label[0:3, 0:4] = 255
    T = np.array([[0.9, 0.2, 3.0], [-0.15, 1.1, -2.0]], dtype=np.float32)
    Tb = np.array([[1.05, 0.0, -1.5], [0.1, 0.95, 2.5]], dtype=np.float32)
    Gs = ('gauss',) + R.blur_spec(2.0, 45)
    for sv in (dict(T=T, G=None, Tb=None, Gb=None), dict(T=T, G=Gs, Tb=Tb, Gb=('gauss',) + R.blur_spec(5.0, 90))):
        want_im, want_lb = aug_ref.augment_ref(image, label[None], [sv], F64)
        p = R.aug_prepare(image, label, F64)
        background = R.pull_push_fill(p['pyr0'], F64)[1]
        inv = warp_ref.inverse_affine(T).ravel()
        wt = R.warp_affine_batch(p['target'], inv, None, 1, (Hh, Ww), F64)
        canvas = background[None]
        if sv['Tb'] is not None:
            canvas = R.warp_affine_batch(background, warp_ref.inverse_affine(Tb).ravel(), [0], 1, (Hh, Ww), F64)
            canvas = R.blur_gauss2d(canvas[0], *sv['Gb'][1:], dtype=F64)[None]
        if sv['G'] is not None:
            wt = R.blur_gauss2d(wt[0], *sv['G'][1:], dtype=F64)[None]
        planes, counts = R.warp_mask_batch(p['maskf'], inv, (Hh, Ww), F64)
        v, q, lb = R.aug_blend(wt, canvas, planes, [0], F64)
        assert torch.equal(q[0], want_im[1]) and torch.equal(lb, want_lb[1]) and counts == [int(want_lb[1].sum())]
        assert torch.equal(R.q_floor(v).to(torch.uint8), q)
        assert torch.equal(p['label01'][None], want_lb[0]) and torch.equal(want_im[0], image)


def test_small_definitions():
    m = torch.zeros(7, 3)
    assert R.mask_stats(m) == [0, 0, 0, 0, 0]
    m[2, 1], m[5, 0] = 0.3, 2.0
    m[6, 2], m[0, 0] = -1.0, -0.0
    assert R.mask_stats(m) == [2, 2, 3, 6, 5]                      # x in 0..1, y in 2..5 of a 7 x 3 mask
    lab = torch.tensor([[0, 1, 255, 1]], dtype=torch.uint8)
    assert R.label_mask(lab, 255)[0].tolist() == [[0, 0, 1, 0]] and R.label_mask(lab, 0)[1].tolist() == [[1.0, 0.0, 0.0, 0.0]]
    p = R.aug_prepare(torch.full((3, 2, 5), 7, dtype=torch.uint8), torch.tensor([[0, 0, 0, 0, 2], [0, 0, 0, 0, 0]], dtype=torch.uint8))
    assert p['pyr0'][3].tolist() == [[1, 1, 1, 0, 0], [1, 1, 1, 0, 0]] and p['target'][3].tolist() == [[0, 0, 0, 0, 255], [0, 0, 0, 0, 0]]
    f = torch.tensor([[2.0, 0, 1, 0, 0.5, -3], [0, 0, 5, 0, 0, 7]])
    inv = R.aug_inverse(f)
    assert inv[0].tolist() == [0.5, 0, -0.5, 0, 2.0, 6.0] and inv[1].tolist() == [1, 0, 0, 0, 1, 0]
    v = torch.tensor([12.99, 13.0, -4.0, 255.5, 254.5, 0.5, 0.49])
    assert R.q_floor(v).tolist() == [12, 13, 0, 255, 254, 0, 0] and R.q_round(v).tolist() == [13, 13, 0, 255, 255, 1, 0]
    assert torch.equal(R.q_round(v).to(torch.uint8), R.round_u8(v))


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact-transform set
# ---------------------------------------------------------------------------------------------------------------------------------
def _all_warp_sizes():
    return R.WARP_SIZES + [R.WARP_LARGE[:2], ((33, 47), (363, 362))]


def test_exact_transform_set_is_exact_in_fp32():
    names = None
    for (Hs, Ws), (Hd, Wd) in _all_warp_sizes():
        ts = R.exact_transforms(Hs, Ws, Hd, Wd)
        names = [n for n, _ in ts]
        for name, fwd in ts:
            a, b, tx, c, d, ty = (float(v) for v in fwd)
            assert {abs(v) for v in (a, b, c, d)} <= {0.0, 0.5, 1.0, 2.0}, name
            det = a * d - b * c
            assert det != 0 and np.log2(abs(det)) == round(np.log2(abs(det))), name
            assert (tx * 4) % 1 == 0 and (ty * 4) % 1 == 0, name
            inv32 = R.invert32(fwd)
            inv64 = warp_ref.inverse_affine(fwd.reshape(2, 3)).ravel()
            assert np.array_equal(inv32.astype(np.float64), inv64), name                     # the host inversion is exact
            sx32, sy32 = R.source_coords(inv32, (Hd, Wd), torch.float32)
            sx64, sy64 = R.source_coords(inv64, (Hd, Wd), F64)
            assert torch.equal(sx32.double(), sx64) and torch.equal(sy32.double(), sy64), name
            assert bool(((sx64 * 4) % 1 == 0).all()) and bool(((sy64 * 4) % 1 == 0).all()), name     # multiples of 1/4 (warp_source_u8)
            if name == 'shift_half':
                assert bool(((sx64 % 1) == 0.5).all()) and bool(((sy64 % 1) == 0.5).all())
            if name == 'one_row_one_column':
                inside = (sx64 >= 0) & (sx64 < Ws) & (sy64 >= 0) & (sy64 < Hs)
                assert int(inside.sum()) == 1 and float(sx64[inside]) == 0 and float(sy64[inside]) == 0
            if name == 'nothing_inside':
                assert float(sx64.max()) <= -3
    for need in ('identity', 'shift_int', 'shift_half', 'flip_lr', 'rot90', 'scale2', 'scale_half', 'shear_b', 'shear_c', 'one_row_one_column',
                 'nothing_inside'):
        assert need in names


@pytest.mark.parametrize('mode', R.MODES)
def test_every_coefficient_of_the_inverse_matters(mode):
    """Perturbing any one of the six inverse coefficients, or swapping any two, changes the reference output of at least one case."""
    cases = []
    for (Hs, Ws), (Hd, Wd) in R.WARP_SIZES[:2]:
        src = R.warp_source_f32(1, Hs, Ws)
        for name, fwd in R.exact_transforms(Hs, Ws, Hd, Wd):
            inv = R.invert32(fwd).astype(np.float64)
            cases.append((src, inv, (Hd, Wd), R.warp_affine(src, inv, (Hd, Wd), mode, F64)))

    def changes(edit):
        for src, inv, size, base in cases:
            m = inv.copy()
            edit(m)
            if not np.array_equal(m, inv) and not torch.equal(R.warp_affine(src, m, size, mode, F64), base):
                return True
        return False

    def add(k, delta):
        def f(m):
            m[k] += delta
        return f

    def swap(k, l):
        def f(m):
            m[k], m[l] = m[l], m[k]
        return f

    for k in range(6):
        assert changes(add(k, 0.5)) and changes(add(k, -1.0)), k
        for l in range(k + 1, 6):
            assert changes(swap(k, l)), (k, l)


# ---------------------------------------------------------------------------------------------------------------------------------
# no envelope is vacuous: loose elements from the fp32 and float64 legs alone
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Hh,Ww,pattern', R.PP_CASES)
def test_loose_share_pull_push(Hh, Ww, pattern):
    level0 = R.pull_push_level0(Hh, Ww, pattern)
    v64, v32 = R.pull_push_fill(level0, F64)[0][0][:3], R.pull_push_fill(level0, torch.float32)[0][0][:3]
    hole = (level0[3] == 0).expand(3, Hh, Ww)
    share = R.loose_share(v64, v32, R.q_floor, hole)
    print('pull-push %dx%d %s: fp32 leg %.3e from float64, loose %.4f of %d hole values' % (Hh, Ww, pattern, float((v32.double() - v64).abs().max()), share, int(hole.sum())))
    assert share <= R.LOOSE_CAP


@pytest.mark.parametrize('sizes', R.WARP_SIZES + [R.WARP_LARGE[:2]], ids=str)
def test_loose_share_warp_u8(sizes):
    (Hs, Ws), (Hd, Wd) = sizes
    large = sizes == R.WARP_LARGE[:2]
    for C in ((R.WARP_LARGE[2],) if large else (1, 3)):
        src = R.warp_source_u8(C, Hs, Ws, 'bicubic')
        assert int(src.max()) == 255 and (Hs * Ws == 1 or int(src.min()) == 0)
        sat = [False, False]
        for name, fwd in R.exact_transforms(Hs, Ws, Hd, Wd):
            if large and name != R.WARP_LARGE[3]:
                continue
            inv = R.invert32(fwd)
            for mode in R.MODES[1:]:
                src = R.warp_source_u8(C, Hs, Ws, mode)
                v64, v32 = R.warp_affine(src, inv, (Hd, Wd), mode, F64), R.warp_affine(src, inv, (Hd, Wd), mode, torch.float32)
                share = R.loose_share(v64, v32, R.q_round)
                assert share <= R.LOOSE_CAP, (name, mode, C, share)
                sat = [sat[0] or float(v64.min()) < -0.5, sat[1] or float(v64.max()) > 255.5]
        assert Hs * Ws < 35 or sat == [True, True]          # the bicubic overshoot saturates at both ends


@pytest.mark.parametrize('Hh,Ww', R.BLEND_SIZES)
def test_loose_share_blend(Hh, Ww):
    for n in (1, 4):
        wt, canvas, labels, index = R.blend_inputs(n, Hh, Ww, 'random')
        v64, v32 = R.aug_blend(wt, canvas, labels, index, F64)[0], R.aug_blend(wt, canvas, labels, index, torch.float32)[0]
        assert R.loose_share(v64, v32, R.q_floor) <= R.LOOSE_CAP
        assert float(v64.min()) < 0 and float(v64.max()) > 255 or Hh * Ww == 1
