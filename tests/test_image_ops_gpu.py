"""Every kernel of the first-frame augmentation (csrc/image_ops.hip) against its float64 definition (tests/_image_refs.py, pinned to the
oracle by tests/test_image_refs.py), called through the C entry points at the smallest shapes each kernel branches on: the grid-stride
second trips, the LDS-tile tails of the blur and the second trip of its table load, the index list of the batched warp, n = 32 of the
host-matrix label warp, the float-mask path of the mask statistics, pyramids whose ceil-halving goes odd at different levels.

Three rules judge, and no others:
  1. EXACT: integer and selection outputs are equal, no share of exceptions -- mask statistics, every output of frtm_aug_prepare,
     frtm_label_mask and the fills, the label planes and counts of the nearest warps under the exact-transform set, the label copy of the
     blend, the pixels the fill must leave alone.
  2. the project's GATE for float outputs, tests/test_refiner_train_gpu.py::_gate:
         max|hip - ref64| <= max(4 * max|torch32 - ref64|, 1e-6 * max|ref64|)
     with ref64 the definition in float64 on the CPU and torch32 the same expression in fp32 on the GPU, as elementwise operations and sums.
  3. ENVELOPE for quantised outputs: with Q the quantiser, v64 the float64 value before it and tol the bound rule 2 gives for that value,
         Q(v64 - tol) <= hip <= Q(v64 + tol)   at every element;
     Q = floor after clamp (the fill's finest level), truncation after clamp (the blend), round half up after clamp (the uint8 warp).
     An element is loose where the two ends differ; from the two reference legs alone at most 5 % of a case may be loose
     (_image_refs.LOOSE_CAP; tests/test_image_refs.py asserts the same from CPU legs).
No tolerance is fixed in advance beyond these rules.

The exact-transform set (_image_refs.exact_transforms) makes the warps' geometry exact in fp32: the host inversion and every source
coordinate are exactly representable, so the kernel and the float64 reference pick the same taps and only the interpolation arithmetic is
left.  General rotations stay with tests/test_round3_gpu.py.

Output hygiene as in tests/test_solver_kernels_gpu.py: float outputs are NaN-prefilled between two NaN guard bands, uint8 and int32 outputs
sit between guard bands of a sentinel byte / word and are prefilled with it; the bands must be unchanged after the launch; words a launch
must not write are compared bit for bit.

Not exercised: the 11-level cap of the fill pyramid, which needs a side above 2048.

No test here asserts a time.  The module (125 tests) ran in 6.1 to 6.2 s on an MI355X; the slowest test is test_blur_gauss2d[40], 0.75 s
(6561 taps per fp32 leg).  Largest RATIO (hip error / torch32 error) per kernel; ratios above 4 passed on the 1e-6 floor of max|ref|:
    k_pp_down / k_pp_up (levels 1 and up) 1.37   k_blur2d (tables) 1.29, at 1 x 947   k_blur2d (Gaussian) 5.19 (half 8 on a 1 x 1 image:
    3.2e-6 against a floor of 4.1e-5)   k_warp_affine (float) 1.30   k_warp_affine_batch 0.87   k_aug_transforms (inverse) 1.71; its forward
    matrices were equal to float32(ImageAugmenter._transform) in every bit (0 ulp)
Largest share of loose elements in an envelope, and the largest tol: k_pp_up 1.1 % (1030 x 1030, tol 5.1e-3), k_warp_affine (uint8) 1.3 %
(tol 3.5e-4), k_aug_blend 0.06 % (tol 2.8e-4); no element of any case lay outside its envelope.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import _image_refs as R
from test_refiner_train_gpu import _gate

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64
NAN = float('nan')
F64 = torch.float64
SENTINEL = {torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A}


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Buf:
    """A device buffer of `shape` between two guard bands.  float32: NaN guards, NaN-filled (an output) or holding `init`; uint8 / int32:
    guards of the sentinel byte / word, filled with it or holding `init`."""

    def __init__(self, *shape, dtype=torch.float32, init=None):
        if init is not None:
            shape, dtype = tuple(init.shape), init.dtype
        n = int(math.prod(shape))
        self.fill = NAN if dtype == torch.float32 else SENTINEL[dtype]
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(init)
        self.before = self.t.clone()
        assert self.t.is_contiguous()

    def _untouched(self, x):
        return bool(torch.isnan(x).all()) if self.fill != self.fill else bool((x == self.fill).all())

    def guards(self):
        torch.cuda.synchronize()
        assert self._untouched(self.buf[:GUARD]), 'write below the buffer'
        assert self._untouched(self.buf[GUARD + self.t.numel():]), 'write above the buffer'

    def done(self):
        """The guards are untouched and (float) every element was written; returns the buffer."""
        self.guards()
        if self.fill != self.fill:
            assert not bool(torch.isnan(self.t).any()), 'output element not written'
        return self.t

    def same(self):
        """The guards and every word are what they were before the launch, bit for bit."""
        self.guards()
        assert torch.equal(self.t.view(torch.uint8), self.before.view(torch.uint8)), 'a word that the launch must not write has changed'
        return self.t


def _call(name, *args):
    from frtm_vos_amd import _hip as H
    H.call(name, *[H.ptr(a) if torch.is_tensor(a) else a for a in args])


def _refused(match, name, *args, keep=()):
    """The argument check refuses the call (it returns before any launch); `keep`: buffers that must be as they were."""
    with pytest.raises(RuntimeError, match=match):
        _call(name, *args)
    for b in keep:
        b.same()


def _d(t):
    return None if t is None else t.to(DEV)


def _host6(mats):
    a = np.ascontiguousarray(np.asarray(mats, dtype=np.float32).reshape(-1))
    return (ctypes.c_float * a.size)(*[float(v) for v in a])


def _check(kernel, case, hip, ref64, t32):
    """Rule 2, with the figures printed first (`pytest -s` shows them)."""
    r = ref64.double().cpu()
    e = float((hip.double().cpu() - r).abs().max())
    e32 = float((t32.double().cpu() - r).abs().max())
    print('RATIO %s %s hip %.3e torch32 %.3e ratio %.3f max|ref| %.3e' % (kernel, case, e, e32, e / max(e32, 1e-30) if e else 0.0, float(r.abs().max())))
    assert tuple(hip.shape) == tuple(ref64.shape)
    _gate(hip, r, t32, '%s %s' % (kernel, case))


def _check_envelope(kernel, case, hip_q, v64, t32, q, where=None):
    """Rule 3 on the elements of `where` (all by default): the cap on loose elements from the two reference legs, then the envelope."""
    v64 = v64.double().cpu()
    tol = R.gate_tol(v64, t32)
    lo, hi, loose = R.envelope(v64, tol, q)
    got = hip_q.double().cpu()
    assert tuple(got.shape) == tuple(v64.shape)
    if where is not None:
        lo, hi, loose, got = lo[where], hi[where], loose[where], got[where]
    share = float(loose.double().mean()) if loose.numel() else 0.0
    outside = int(((got < lo) | (got > hi)).sum())
    print('ENVELOPE %s %s tol %.3e loose %.4f of %d outside %d high-end %d' % (kernel, case, tol, share, loose.numel(), outside, int((loose & (got == hi)).sum())))
    assert share <= R.LOOSE_CAP, '%s %s: %.3f of the elements are loose, the envelope says too little' % (kernel, case, share)
    assert outside == 0, '%s %s: %d elements outside [Q(v - tol), Q(v + tol)], tol %.3e' % (kernel, case, outside, tol)


# ---------------------------------------------------------------------------------------------------------------------------------
# frtm_mask_stats, frtm_aug_prepare, frtm_label_mask, fill32
# ---------------------------------------------------------------------------------------------------------------------------------
def _stat_masks(Hh, Ww):
    def m(*pix):
        t = torch.zeros(Hh, Ww, dtype=torch.bool)
        for y, x in pix:
            t[y, x] = True
        return t
    blobs = torch.zeros(Hh, Ww, dtype=torch.bool)
    blobs[Hh // 8:Hh // 8 + max(1, Hh // 5), Ww // 7:Ww // 7 + max(1, Ww // 4)] = True
    blobs[Hh - 1 - Hh // 3:Hh - Hh // 6, Ww - 1 - Ww // 5:Ww - Ww // 9] = True
    return [('empty', m()), ('top_left', m((0, 0))), ('top_right', m((0, Ww - 1))), ('bottom_left', m((Hh - 1, 0))),
            ('bottom_right', m((Hh - 1, Ww - 1))), ('full', torch.ones(Hh, Ww, dtype=torch.bool)), ('two_blobs', blobs)]


@pytest.mark.parametrize('as_u8', [True, False], ids=['uint8', 'float'])
@pytest.mark.parametrize('Hh,Ww', [(1, 1), (7, 3), (33, 47), (257, 256)])
def test_mask_stats(Hh, Ww, as_u8):
    """(257, 256) is one pixel row more than 256 blocks of 256 cover: the second trip.  Float masks hold 0.3 and 2 where set and
    -1, -0.0 and 0 elsewhere: only values > 0 count."""
    g = R.gen(Hh, Ww, 21)
    for name, on in _stat_masks(Hh, Ww):
        if as_u8:
            mask = torch.where(on, torch.randint(1, 256, (Hh, Ww), generator=g), torch.zeros(Hh, Ww, dtype=torch.long)).to(torch.uint8)
        else:
            off = torch.tensor([-1.0, -0.0, 0.0])[torch.randint(0, 3, (Hh, Ww), generator=g)]
            mask = torch.where(on, torch.tensor([0.3, 2.0])[torch.randint(0, 2, (Hh, Ww), generator=g)], off)
        out = _Buf(5, dtype=torch.int32)
        _call('frtm_mask_stats', _d(mask), int(as_u8), Hh, Ww, out.t)
        want = R.mask_stats(mask)
        assert want[0] == int(on.sum()) and (name != 'empty' or want == [0] * 5)
        assert out.done().tolist() == want, (name, out.t.tolist(), want)


def _border_label(Hh, Ww, g):
    """Set pixels on all four borders (the 3x3 dilation is clipped there), values 1, 2 and 255, and a blob inside."""
    lb = torch.zeros(Hh, Ww, dtype=torch.uint8)
    lb[0, Ww // 3:Ww // 3 + max(1, Ww // 4)] = 2
    lb[Hh - 1, Ww // 2:] = 255
    lb[Hh // 4:Hh // 4 + max(1, Hh // 5), 0] = 1
    lb[Hh // 2:Hh // 2 + max(1, Hh // 6), Ww - 1] = 2
    lb[Hh // 3:Hh // 3 + max(1, Hh // 4), Ww // 5:Ww // 5 + max(1, Ww // 3)] = 255
    lb[Hh - 1, 0] = 0 if Hh * Ww > 1 else 2
    return lb


@pytest.mark.parametrize('with_label01', [True, False])
@pytest.mark.parametrize('Hh,Ww', [(1, 1), (2, 5), (33, 47), (725, 724)])
def test_aug_prepare(Hh, Ww, with_label01):
    """(725, 724) passes the 2048-block cap.  All four outputs are exact: every value is an integer below 2^24."""
    g = R.gen(Hh, Ww, 22)
    image = torch.randint(0, 256, (3, Hh, Ww), generator=g).to(torch.uint8)
    labels = [_border_label(Hh, Ww, g)] + ([torch.zeros(1, 1, dtype=torch.uint8)] if Hh * Ww == 1 else [])
    for lb in labels:
        target, pyr0, maskf = _Buf(4, Hh, Ww), _Buf(4, Hh, Ww), _Buf(Hh, Ww)
        lab01 = _Buf(Hh, Ww, dtype=torch.uint8)
        _call('frtm_aug_prepare', _d(image), _d(lb), Hh, Ww, target.t, pyr0.t, maskf.t, lab01.t if with_label01 else None)
        want = R.aug_prepare(image, lb, F64)
        for name, buf in (('target', target), ('pyr0', pyr0), ('maskf', maskf)):
            assert torch.equal(buf.done().cpu().double(), want[name]), name
        if with_label01:
            assert torch.equal(lab01.done().cpu(), want['label01'])
        else:
            lab01.same()
        if Hh * Ww > 10:
            assert set(lb.unique().tolist()) == {0, 1, 2, 255}
            assert float(want['pyr0'][3].min()) == 0 and float(want['pyr0'][3].max()) == 1


@pytest.mark.parametrize('with_plane', [True, False])
@pytest.mark.parametrize('n', [1, 257, 1024 * 256 + 3])
def test_label_mask(n, with_plane):
    """1024 * 256 + 3 labels pass the 1024-block cap."""
    labels = torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=R.gen(n, 23))]
    src = _Buf(init=labels)
    for obj_id in (0, 1, 255):
        mask, plane = _Buf(n, dtype=torch.uint8), _Buf(n)
        _call('frtm_label_mask', src.t, obj_id, n, mask.t, plane.t if with_plane else None)
        want_u8, want_f = R.label_mask(labels, obj_id)
        assert torch.equal(mask.done().cpu(), want_u8)
        if with_plane:
            assert torch.equal(plane.done().cpu(), want_f)
        else:
            plane.same()
    src.same()


def test_fill32():
    """_hip.fill: a slice at a word offset, n = 0, a float and an int pattern; the words around the slice stay bit for bit."""
    from frtm_vos_amd import _hip as H
    for dtype, value in ((torch.float32, -1.5), (torch.float32, 0.0), (torch.int32, -7), (torch.int32, 0x12345678)):
        for lo, n in ((0, 1), (3, 0), (3, 5), (1, 1024 * 256 + 3)):
            init = torch.randint(-1000, 1000, (lo + n + 6,), generator=R.gen(lo, n, 24)).to(dtype)
            buf = _Buf(init=init)
            H.fill(buf.t[lo:lo + n], value)
            buf.guards()
            want = init.clone()
            want[lo:lo + n] = value
            assert torch.equal(_bits(buf.t.cpu()), _bits(want)), (dtype, value, lo, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# frtm_pull_push_fill
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('Hh,Ww,pattern', R.PP_CASES)
def test_pull_push_fill(Hh, Ww, pattern):
    """Levels 1 and up by rule 2 (they stay unfloored in the pyramid buffer, at the offsets frtm_pull_push_elems implies), the finest level's
    hole pixels by rule 3, its known pixels and its known plane by rule 1.  (2, 7) has no level below the image: the buffer is unchanged.
    The image values carry fractions (_image_refs.pull_push_image says why); a second launch on integer values checks rule 1 alone."""
    from frtm_vos_amd import _hip as H
    elems = int(H.lib().frtm_pull_push_elems(Hh, Ww))
    assert elems == R.pull_push_elems(Hh, Ww)
    level0 = R.pull_push_level0(Hh, Ww, pattern)
    pyr = _Buf(elems)
    pyr.t[:level0.numel()] = level0.reshape(-1).to(DEV)
    pyr.before = pyr.t.clone()
    _call('frtm_pull_push_fill', pyr.t, elems, Hh, Ww)
    sizes = R.pull_push_sizes(Hh, Ww)
    if len(sizes) == 1:
        pyr.same()
        return
    out = pyr.done().cpu()
    l64, _ = R.pull_push_fill(level0, F64)
    l32, _ = R.pull_push_fill(level0.to(DEV), torch.float32)
    case = '%dx%d %s' % (Hh, Ww, pattern)
    off = 0
    for l, (h, w) in enumerate(sizes):
        got = out[off:off + 4 * h * w].view(4, h, w)
        off += 4 * h * w
        assert torch.equal(got[3].double(), l64[l][3]), 'known plane of level %d' % l
        if l > 0:
            _check('k_pp_down/k_pp_up', '%s level %d' % (case, l), got[:3], l64[l][:3], l32[l][:3])
    assert off == elems
    fin = out[:4 * Hh * Ww].view(4, Hh, Ww)
    known = level0[3] > 0
    assert torch.equal(_bits(fin[:3][:, known]), _bits(level0[:3][:, known].floor())), 'a known pixel is not its own value floored'
    assert torch.equal(_bits(fin[3]), _bits(level0[3]))
    _check_envelope('k_pp_up', case, fin[:3], l64[0][:3], l32[0][:3], R.q_floor, where=(~known).expand(3, Hh, Ww))
    if pattern == 'nothing_known':
        assert float(out.abs().max()) == 0.0
    # integer image values, what frtm_aug_prepare leaves: the fill leaves known pixels and the known plane alone, bit for bit
    level0 = R.pull_push_level0(Hh, Ww, pattern, integer=True)
    pyr = _Buf(elems)
    pyr.t[:level0.numel()] = level0.reshape(-1).to(DEV)
    _call('frtm_pull_push_fill', pyr.t, elems, Hh, Ww)
    fin = pyr.done().cpu()[:4 * Hh * Ww].view(4, Hh, Ww)
    assert torch.equal(_bits(fin[:3][:, known]), _bits(level0[:3][:, known])), 'a known pixel changed'
    assert torch.equal(_bits(fin[3]), _bits(level0[3]))
    assert bool((fin[:3] == fin[:3].floor()).all()) and float(fin[:3].min()) >= 0 and float(fin[:3].max()) <= 255


# ---------------------------------------------------------------------------------------------------------------------------------
# frtm_blur2d, frtm_blur_gauss2d
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('planes', [1, 4])
@pytest.mark.parametrize('Hh,Ww', R.BLUR_IMAGES)
def test_blur2d_tables(planes, Hh, Ww):
    """Random signed tables; 17 x 17 = 289 taps take the second trip of the table load; 15 x 17 and 33 x 47 leave partial tiles."""
    for kh, kw in R.BLUR_TABLES:
        g = R.gen(planes, Hh, Ww, kh, kw)
        x, G = torch.randn(planes, Hh, Ww, generator=g) * 50, torch.randn(kh, kw, generator=g)
        src, out = _Buf(init=x), _Buf(planes, Hh, Ww)
        _call('frtm_blur2d', src.t, planes, Hh, Ww, _d(G), kh, kw, out.t)
        _check('k_blur2d', 'table %dx%d image %dx%dx%d' % (kh, kw, planes, Hh, Ww), out.done(), R.blur2d(x, G, F64), R.blur2d(_d(x), _d(G), torch.float32))
        src.same()


@pytest.mark.parametrize('half', R.BLUR_HALVES)
def test_blur_gauss2d(half):
    """The reference is oracle.aug_ref.gauss_blur_ref in float64; the fp32 leg is the tap form.  half = 40 (6561 taps per leg) runs one
    image and every third (qa, qb, qc) plus the isotropic wide one, the only one whose far taps weigh anything."""
    wide = half > 8
    qs = R.BLUR_Q[::3] if wide else R.BLUR_Q
    assert R.BLUR_Q[-1] in qs
    for qi, (qa, qb, qc) in enumerate(qs):
        for k, (Hh, Ww) in enumerate(R.BLUR_IMAGES[-1:] if wide else R.BLUR_IMAGES):
            planes = 4 if (qi + k) % 2 or wide else 1
            x = torch.randn(planes, Hh, Ww, generator=R.gen(half, qi, Hh, Ww)) * 50 + 100
            src, out = _Buf(init=x), _Buf(planes, Hh, Ww)
            _call('frtm_blur_gauss2d', src.t, planes, Hh, Ww, half, qa, qb, qc, out.t)
            _check('k_blur2d(gauss)', 'half %d q (%.3g, %.3g, %.3g) image %dx%dx%d' % (half, qa, qb, qc, planes, Hh, Ww), out.done(),
                   R.blur_gauss2d(x, half, qa, qb, qc, F64), R.blur_gauss2d(_d(x), half, qa, qb, qc, torch.float32, taps=True))
            src.same()


def test_blur_lds_limit():
    """The kernel's 64 static bytes count against the 64 KB of a launch: a 1 x 949 table (65492 dynamic bytes) is refused by the argument
    check, a 1 x 947 table (65356) runs."""
    Hh, Ww = 15, 17
    g = R.gen(947)
    x = torch.randn(1, Hh, Ww, generator=g) * 50
    out = _Buf(1, Hh, Ww)
    _refused('too large for the LDS tile', 'frtm_blur2d', _d(x), 1, Hh, Ww, _d(torch.randn(1, 949, generator=g)), 1, 949, out.t, keep=(out,))
    _refused('too large for the LDS tile', 'frtm_blur2d', _d(x), 1, Hh, Ww, _d(torch.randn(3, 767, generator=g)), 3, 767, out.t, keep=(out,))
    G = torch.randn(1, 947, generator=g)
    _call('frtm_blur2d', _d(x), 1, Hh, Ww, _d(G), 1, 947, out.t)
    _check('k_blur2d', 'table 1x947', out.done(), R.blur2d(x, G, F64), R.blur2d(_d(x), _d(G), torch.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# frtm_warp_affine, frtm_warp_affine_u8
# ---------------------------------------------------------------------------------------------------------------------------------
def _warp_case(C, Hs, Ws, Hd, Wd, name, fwd, modes=R.MODES):
    inv = R.invert32(fwd)
    for u8 in (False, True):
        for mode in modes:
            src = R.warp_source_u8(C, Hs, Ws, mode) if u8 else R.warp_source_f32(C, Hs, Ws)
            sbuf = _Buf(init=src)
            out = _Buf(C, Hd, Wd, dtype=src.dtype)
            _call('frtm_warp_affine_u8' if u8 else 'frtm_warp_affine', sbuf.t, C, Hs, Ws, out.t, Hd, Wd, _host6(fwd), R.MODES.index(mode))
            got = out.done()
            v64 = R.warp_affine(src, inv, (Hd, Wd), mode, F64)
            case = '%s %s %s C%d %dx%d->%dx%d' % ('u8' if u8 else 'f32', mode, name, C, Hs, Ws, Hd, Wd)
            sbuf.same()
            if mode == 'nearest':
                assert torch.equal(got.cpu().double(), v64), case
                continue
            v32 = R.warp_affine(_d(src), inv, (Hd, Wd), mode, torch.float32)
            if u8:
                _check_envelope('k_warp_affine', case, got, v64, v32, R.q_round)
            else:
                _check('k_warp_affine', case, got, v64, v32)
            if name == 'nothing_inside':
                assert int((got != 0).sum()) == 0


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('sizes', R.WARP_SIZES, ids=str)
def test_warp_affine_exact_set(sizes, C):
    """All three modes on the exact-transform set, float and uint8: nearest by rule 1, float bilinear and bicubic by rule 2, uint8 by rule 3."""
    (Hs, Ws), (Hd, Wd) = sizes
    for name, fwd in R.exact_transforms(Hs, Ws, Hd, Wd):
        _warp_case(C, Hs, Ws, Hd, Wd, name, fwd)


def test_warp_affine_second_trip():
    """3 x 600 x 600 outputs are more than 4096 blocks of 256 cover."""
    (Hs, Ws), (Hd, Wd), C, name = R.WARP_LARGE
    assert C * Hd * Wd > 4096 * 256
    _warp_case(C, Hs, Ws, Hd, Wd, name, dict(R.exact_transforms(Hs, Ws, Hd, Wd))[name])


# ---------------------------------------------------------------------------------------------------------------------------------
# frtm_warp_mask_batch, frtm_warp_mask_batch_dev, frtm_warp_affine_batch
# ---------------------------------------------------------------------------------------------------------------------------------
def _transform_list(n, Hs, Ws, Hd, Wd):
    """n forward matrices: the exact-transform set, repeated with further integer shifts."""
    base = R.exact_transforms(Hs, Ws, Hd, Wd)
    out = []
    for j in range(n):
        m = base[j % len(base)][1].copy()
        m[2] += 3 * (j // len(base))
        m[5] -= 2 * (j // len(base))
        out.append(m)
    return np.stack(out)


def _mask_source(Hs, Ws):
    """A float mask plane: 0.3 and 1 where set; 0, -0.0 and -1 elsewhere."""
    g = R.gen(Hs, Ws, 31)
    on = torch.rand(Hs, Ws, generator=g) < 0.4
    on[Hs // 4:Hs // 2 + 1, Ws // 4:Ws // 2 + 1] = True
    return torch.where(on, torch.tensor([0.3, 1.0])[torch.randint(0, 2, (Hs, Ws), generator=g)], torch.tensor([0.0, -0.0, -1.0])[torch.randint(0, 3, (Hs, Ws), generator=g)])


MASK_BATCH = [(1, (20, 61)), (19, (20, 61)), (32, (20, 61)), (19, (363, 362))]          # 363 x 362 passes the 512-block cap


def _check_planes(planes, counts, src, inv, size, n):
    want, want_counts = R.warp_mask_batch(src, inv, size, F64)
    got = planes.done().cpu()
    assert torch.equal(got, want)
    assert counts == want_counts and counts == [int(p.sum()) for p in got]
    assert sum(counts) > 0 and (n < 12 or 0 in counts)          # 'nothing_inside' gives an empty plane


@pytest.mark.parametrize('n,size', MASK_BATCH, ids=str)
def test_warp_mask_batch(n, size):
    Hs, Ws = 33, 47
    src, fwd = _mask_source(Hs, Ws), _transform_list(n, 33, 47, *size)
    planes, counts = _Buf(n, *size, dtype=torch.uint8), _Buf(n, dtype=torch.int32)
    _call('frtm_warp_mask_batch', _d(src), Hs, Ws, planes.t, size[0], size[1], _host6(fwd), n, counts.t)
    _check_planes(planes, counts.done().tolist(), src, np.stack([R.invert32(f) for f in fwd]), size, n)


@pytest.mark.parametrize('n,size', MASK_BATCH + [(33, (20, 61))], ids=str)
def test_warp_mask_batch_dev(n, size):
    """The inverses in device memory, no limit of 32, the counts at an offset in a caller's record (the product passes rec + 20 bytes)."""
    Hs, Ws = 33, 47
    src = _mask_source(Hs, Ws)
    inv = np.stack([R.invert32(f) for f in _transform_list(n, 33, 47, *size)])
    planes = _Buf(n, *size, dtype=torch.uint8)
    rec = _Buf(5 + n + 3, dtype=torch.int32)
    inv_dev = _Buf(init=torch.from_numpy(inv))
    _call('frtm_warp_mask_batch_dev', _d(src), Hs, Ws, planes.t, size[0], size[1], inv_dev.t, n, rec.t.data_ptr() + 20)
    words = rec.done().tolist()
    assert words[:5] == [SENTINEL[torch.int32]] * 5 and words[5 + n:] == [SENTINEL[torch.int32]] * 3
    _check_planes(planes, words[5:5 + n], src, inv, size, n)
    inv_dev.same()


@pytest.mark.parametrize('C,n,index,size', [(3, 1, None, (20, 61)), (4, 5, None, (20, 61)), (3, 5, [4, 0, 6, 2, 5], (20, 61)), (4, 5, [1, 3, 3, 7, 1], (9, 4)),
                                            (4, 1, [2], (20, 61)), (4, 2, [6, 4], (363, 362))], ids=str)
def test_warp_affine_batch(C, n, index, size):
    """Bicubic, clamped to [0, 255]; the inverse of launch j is inv[index[j]] (a permutation, a list with repeated entries) or inv[j].
    4 x 363 x 362 passes the 2048-block cap.  Rule 2 on the exact-transform set."""
    Hs, Ws = (33, 47) if size != (9, 4) else (5, 7)
    names = ['shift_half', 'scale2', 'shear_b', 'shift_quarter', 'scale_half', 'rot90', 'flip_lr', 'shear_c']
    ts = dict(R.exact_transforms(Hs, Ws, *size))
    inv = np.stack([R.invert32(ts[k]) for k in names])
    src = R.warp_source_f32(C, Hs, Ws)
    out, inv_dev = _Buf(n, C, *size), _Buf(init=torch.from_numpy(inv))
    idx = None if index is None else _Buf(init=torch.tensor(index, dtype=torch.int32))
    _call('frtm_warp_affine_batch', _d(src), C, Hs, Ws, out.t, size[0], size[1], inv_dev.t, None if idx is None else idx.t, n)
    r64 = R.warp_affine_batch(src, inv, index, n, size, F64)
    r32 = R.warp_affine_batch(_d(src), inv, index, n, size, torch.float32)
    assert float(r64.min()) == 0.0 and float(r64.max()) == 255.0          # both ends of the clamp bind
    _check('k_warp_affine_batch', 'C%d n%d index %s %dx%d' % (C, n, index, size[0], size[1]), out.done(), r64, r32)
    inv_dev.same()
    if idx is not None:
        idx.same()


# ---------------------------------------------------------------------------------------------------------------------------------
# frtm_aug_blend
# ---------------------------------------------------------------------------------------------------------------------------------
def _blend(n, Hh, Ww, alpha):
    wt, canvas, labels, index = R.blend_inputs(n, Hh, Ww, alpha)
    out_im, out_lb = _Buf(n, 3, Hh, Ww, dtype=torch.uint8), _Buf(n, Hh, Ww, dtype=torch.uint8)
    bufs = [_Buf(init=wt), _Buf(init=canvas), _Buf(init=labels), _Buf(init=torch.tensor(index, dtype=torch.int32))]
    _call('frtm_aug_blend', bufs[0].t, bufs[1].t, n, Hh, Ww, bufs[2].t, bufs[3].t, out_im.t, out_lb.t)
    im, lb = out_im.done().cpu(), out_lb.done().cpu()
    for b in bufs:
        b.same()
    assert torch.equal(lb, labels[torch.tensor(index)])          # the label copy through the index list, exact
    return wt, canvas, labels, index, im


@pytest.mark.parametrize('alpha', ['zero', 'one'])
@pytest.mark.parametrize('n', [1, 4])
@pytest.mark.parametrize('Hh,Ww', R.BLEND_SIZES)
def test_aug_blend_exact_alpha(Hh, Ww, n, alpha):
    """Alpha plane exactly 0 / 255: the output is the canvas / the target, clamped to [0, 255] and TRUNCATED (12.99 -> 12, 254.999 -> 254,
    -0.5 -> 0, 255.5 -> 255), exactly.  (513, 512) passes the 1024-block cap."""
    wt, canvas, labels, index, im = _blend(n, Hh, Ww, alpha)
    chosen = wt[:, :3] if alpha == 'one' else canvas
    assert float(chosen.reshape(-1)[0]) == pytest.approx(12.99 if alpha == 'one' or Hh * Ww == 1 else 0.999)
    assert torch.equal(im, chosen.clamp(0, 255).floor().to(torch.uint8))
    assert torch.equal(im, R.aug_blend(wt, canvas, labels, index, F64)[1])
    if alpha == 'one':
        assert int(im.reshape(n, 3, -1)[0, 0, 0]) == 12
    assert Hh * Ww == 1 or (float(chosen.min()) < 0 and float(chosen.max()) > 255)


@pytest.mark.parametrize('n', [1, 4])
@pytest.mark.parametrize('Hh,Ww', R.BLEND_SIZES)
def test_aug_blend_fractional_alpha(Hh, Ww, n):
    wt, canvas, labels, index, im = _blend(n, Hh, Ww, 'random')
    v64 = R.aug_blend(wt, canvas, labels, index, F64)[0]
    v32 = R.aug_blend(_d(wt), _d(canvas), _d(labels), index, torch.float32)[0]
    _check_envelope('k_aug_blend', 'n%d %dx%d' % (n, Hh, Ww), im, v64, v32, R.q_floor)


# ---------------------------------------------------------------------------------------------------------------------------------
# frtm_aug_transforms
# ---------------------------------------------------------------------------------------------------------------------------------
def _transform_specs(n):
    """(spec, limit_scale) pairs that take every branch of k_aug_transforms: a scale relative to the target height, a scale the limit cuts
    (too large, too small), a flip, limit_scale off, and scale 0 (limit off), whose forward matrix has determinant 0."""
    base = [(dict(scale='0.5'), True), (dict(scale=50.0), True), (dict(scale=0.01), True), (dict(scale=1.5, fliplr=True), True),
            (dict(scale=50.0), False), (dict(scale=0.0), False), (dict(scale='1.0', fliplr=True), True), (dict(scale=0.7), True)]
    rot, skew = [0, 5, -10, 20, -30, 45, 60, 90, -45], [(0.0, 0.0), (0.1, 0.1), (0.3, -0.2)]
    loc = [(0.5, 0.5), (0.211, 0.703), (0.9, 0.125)]
    out = []
    for j in range(n):
        s, lim = base[j % len(base)]
        out.append((dict(s, rotation=rot[(j // 2) % len(rot)], skew=skew[(j // 3) % len(skew)], location=loc[(j // 5) % len(loc)], min_size=10 + j % 3), lim))
    return out


@pytest.mark.parametrize('n', [1, 64, 65])
def test_aug_transforms(n):
    """One block of 64 threads holds 64 specs: n = 65 takes a second block.  Forward: float32(ImageAugmenter._transform) within 1 fp32 ulp (the
    device composes the same float64 product in another order).  Inverse: rule 2 against the float64 inverse of the fp32 forward."""
    from frtm_vos_amd.model.augmenter import ImageAugmenter as A
    Hh, Ww = 120, 214
    lb = torch.zeros(Hh, Ww, dtype=torch.uint8)
    lb[30:71, 80:133] = 1
    lb[25:30, 90:95] = 1
    stats = _Buf(5, dtype=torch.int32)
    _call('frtm_mask_stats', _d(lb), 1, Hh, Ww, stats.t)
    n_px, box = A._decode_stats(stats.done().tolist(), (Hh, Ww))
    stats.before = stats.t.clone()
    assert n_px == int(lb.sum()) and box == (80 + 53 / 2, 25 + 46 / 2, 53, 46)
    specs = _transform_specs(n if n > 1 else 8)
    for first in (range(8) if n == 1 else [0]):          # n = 1: every branch in a launch of its own
        chunk = specs[first:first + n]
        rows = torch.tensor([A._spec_row(s, lim) for s, lim in chunk], dtype=torch.float64).to(DEV)
        fwd, inv = _Buf(n, 6), _Buf(n, 6)
        _call('frtm_aug_transforms', rows, n, stats.t, Hh, Ww, fwd.t, inv.t)
        f = fwd.done().cpu()
        want = np.stack([np.asarray(A._transform(s, box, (Hh, Ww), limit_scale=lim)[0], dtype=np.float64)[:2].ravel() for s, lim in chunk]).astype(np.float32)
        ulps = np.abs(f.numpy().astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(np.abs(want), np.abs(f.numpy())))
        print('FORWARD n%d first %d: largest difference %.2f ulp' % (n, first, float(ulps.max())))
        assert float(ulps.max()) <= 1.0, (first, ulps.max())
        singular = [(f[j, 0] * f[j, 4] - f[j, 1] * f[j, 3]) == 0 for j in range(n)]
        assert [j for j in range(n) if singular[j]] == [j for j, (s, _) in enumerate(chunk) if s['scale'] == 0.0]
        got = inv.done()
        for j in range(n):
            if singular[j]:
                assert got[j].tolist() == [1, 0, 0, 0, 1, 0]
        _check('k_aug_transforms', 'inverse n%d first %d' % (n, first), got, R.aug_inverse(f, F64), R.aug_inverse(_d(f), torch.float32))
        stats.same()


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: argument checks, which return before any launch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    Hs, Ws, Hd, Wd = 5, 7, 9, 4
    x, xu = _d(torch.ones(1, Hs, Ws)), _d(torch.ones(1, Hs, Ws, dtype=torch.uint8))
    out, outu = _Buf(1, Hd, Wd), _Buf(1, Hd, Wd, dtype=torch.uint8)
    eye, singular = _host6([1, 0, 0, 0, 1, 0]), _host6([1, 2, 0, 2, 4, 5])
    for name, s, o in (('frtm_warp_affine', x, out), ('frtm_warp_affine_u8', xu, outu)):
        _refused('bad argument', name, None, 1, Hs, Ws, o.t, Hd, Wd, eye, 2, keep=(o,))
        _refused('bad argument', name, s, 1, Hs, Ws, None, Hd, Wd, eye, 2, keep=(o,))
        _refused('bad argument', name, s, 1, Hs, Ws, o.t, Hd, Wd, None, 2, keep=(o,))
        _refused('bad argument', name, s, 0, Hs, Ws, o.t, Hd, Wd, eye, 2, keep=(o,))
        _refused('mode must be', name, s, 1, Hs, Ws, o.t, Hd, Wd, eye, 3, keep=(o,))
        _refused('mode must be', name, s, 1, Hs, Ws, o.t, Hd, Wd, eye, -1, keep=(o,))
        _refused('singular', name, s, 1, Hs, Ws, o.t, Hd, Wd, singular, 1, keep=(o,))
    # the blur: even table sizes, null pointers, half widths whose tile does not fit
    b = _Buf(1, Hs, Ws)
    G = _d(torch.ones(4, 4))
    for kh, kw in ((2, 3), (3, 4), (0, 1)):
        _refused('odd kernel sizes only', 'frtm_blur2d', x, 1, Hs, Ws, G, kh, kw, b.t, keep=(b,))
    _refused('bad argument', 'frtm_blur2d', x, 1, Hs, Ws, None, 3, 3, b.t, keep=(b,))
    _refused('bad argument', 'frtm_blur2d', None, 1, Hs, Ws, G, 3, 3, b.t, keep=(b,))
    _refused('too large for the LDS tile', 'frtm_blur_gauss2d', x, 1, Hs, Ws, 41, 0.1, 0.0, 0.1, b.t, keep=(b,))
    _refused('bad argument', 'frtm_blur_gauss2d', x, 1, Hs, Ws, -1, 0.1, 0.0, 0.1, b.t, keep=(b,))
    _refused('bad argument', 'frtm_blur_gauss2d', x, 1, Hs, Ws, 1, 0.1, 0.0, 0.1, None)
    # the label warps: 1..32 host matrices, a singular one among them, null pointers
    planes, counts = _Buf(33, Hd, Wd, dtype=torch.uint8), _Buf(33, dtype=torch.int32)
    many = _host6([[1, 0, 0, 0, 1, 0]] * 33)
    for n in (0, 33):
        _refused('1..32 transforms', 'frtm_warp_mask_batch', x, Hs, Ws, planes.t, Hd, Wd, many, n, counts.t, keep=(planes, counts))
    _refused('singular transform 1', 'frtm_warp_mask_batch', x, Hs, Ws, planes.t, Hd, Wd, _host6([[1, 0, 0, 0, 1, 0], [0, 0, 1, 0, 0, 1]]), 2, counts.t,
             keep=(planes, counts))
    inv = _d(torch.tensor([[1.0, 0, 0, 0, 1, 0]]))
    _refused('bad argument', 'frtm_warp_mask_batch_dev', x, Hs, Ws, planes.t, Hd, Wd, inv, 0, counts.t, keep=(planes, counts))
    _refused('bad argument', 'frtm_warp_mask_batch_dev', x, Hs, Ws, planes.t, Hd, Wd, None, 1, counts.t, keep=(planes, counts))
    _refused('bad argument', 'frtm_warp_mask_batch_dev', x, Hs, Ws, planes.t, Hd, Wd, inv, 1, None, keep=(planes, counts))
    _refused('bad argument', 'frtm_warp_affine_batch', x, 1, Hs, Ws, out.t, Hd, Wd, inv, None, 0, keep=(out,))
    _refused('bad argument', 'frtm_warp_affine_batch', x, 1, Hs, Ws, out.t, Hd, Wd, None, None, 1, keep=(out,))
    # the fill: a pyramid buffer one float short
    elems = R.pull_push_elems(17, 33)
    pyr = _Buf(init=torch.ones(elems))
    _refused('the pyramid needs %d floats' % elems, 'frtm_pull_push_fill', pyr.t, elems - 1, 17, 33, keep=(pyr,))
    _refused('bad argument', 'frtm_pull_push_fill', None, elems, 17, 33)
    # the rest: null pointers and empty sizes
    st = _Buf(5, dtype=torch.int32)
    _refused('bad argument', 'frtm_mask_stats', None, 1, Hs, Ws, st.t, keep=(st,))
    _refused('bad argument', 'frtm_mask_stats', xu, 1, 0, Ws, st.t, keep=(st,))
    _refused('bad argument', 'frtm_aug_prepare', xu, None, Hs, Ws, out.t, out.t, out.t, None, keep=(out,))
    _refused('bad argument', 'frtm_aug_blend', x, x, 1, Hs, Ws, xu, None, outu.t, outu.t, keep=(outu,))
    _refused('bad argument', 'frtm_aug_blend', x, x, 0, Hs, Ws, xu, _d(torch.zeros(1, dtype=torch.int32)), outu.t, outu.t, keep=(outu,))
    _refused('bad argument', 'frtm_label_mask', xu, 256, Hs * Ws, outu.t, None, keep=(outu,))
    _refused('bad argument', 'frtm_label_mask', xu, 1, 0, outu.t, None, keep=(outu,))
    _refused('bad argument', 'frtm_aug_transforms', _d(torch.zeros(10, dtype=F64)), 0, st.t, Hs, Ws, out.t, out.t, keep=(st, out))
    _refused('bad argument', 'frtm_aug_transforms', None, 1, st.t, Hs, Ws, out.t, out.t, keep=(st, out))
    from frtm_vos_amd import _hip as H
    with pytest.raises(RuntimeError, match='null pointer'):
        H.call('frtm_fill32', None, 4, 0)
