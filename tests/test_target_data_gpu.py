"""What feeds the target-model solver -- the memory and gradient half of csrc/target_model.hip: pixel weights, the low-resolution normal
equations, the sample-weight and slot logic of the memory, the inserts, the window update, the filter weight and input gradients, the pitched
score writer, the transpose, the guarded roll-back copy, the stand-alone mask merge and the pixel count -- against its float64 definition
(tests/_target_refs.py and, for the gradients and the stencil, tests/_solver_refs.py; pinned by tests/test_target_refs.py and
tests/test_solver_refs.py), called through the C entry points at the shapes the kernels branch on.

The apparatus is that of tests/test_solver_kernels_gpu.py: the gate tests/test_refiner_train_gpu.py::_gate,
    max|hip - ref64| <= max(4 * max|torch32 - ref64|, 1e-6 * max|ref64|),
the three legs reading the same fp32 values of a seeded CPU generator (tf, lr and the merge's clamp bounds as the fp32 values the kernels hold);
every output NaN-filled between two guard bands of 64 floats (_Buf: done() = every word written, same() = no word changed, bit for bit); integer
outputs between guard bands of a sentinel (_IntBuf) and compared exactly; `RATIO` printed for each check (`pytest -s`).

Which branch each shape reaches:
  k_label_sum / k_pixel_weights_map   1 x 1 and 3 x 5: fewer pixels than the 32 parts, so empty parts, which must be written (as zeros); 7 x 9: no
                                      multiple of 32; 363 x 362 = 131406 pixels > 512 x 256: the second grid-stride trip of the map kernel.  9 and
                                      10 foreground pixels: both sides of the `px < 10` rule (test_target_refs.py: the weights differ by > 1e-3);
                                      a fraction below and above tf; tf = -1.  The kernel sums the raw label values where frtm_normal_build
                                      thresholds them: the two agree for labels in {0, 1} only, which is what is pinned here.
  k_normal_build                      8 -> 8: the identity; 12 x 40 -> 1 x 5 and 40 x 12 -> 5 x 1: a cell that is first and last at once; 37 x 53 ->
                                      5 x 7: a non-integer ratio; 50 x 120 -> 3 x 3: fx = 40, the middle cell's window is 83 columns: the second
                                      64-lane trip, and 9 cells: a block with one live wave; 90 x 20 -> 3 x 2: several 20-row blocks with a tail;
                                      64 -> 2; 9 x 10 -> 8 x 9: a ratio just above 1.  Each of the nine tap planes and c gated on its own.  slot_host, slot_dev >= 0 and -1; the slot
                                      table with a repeated slot through frtm_memory_update_window.
  next_slot_step                      cap 5 / 64 / 65 / 130: one trip with idle lanes, one full trip, a second trip of one lane, a third trip;
                                      every branch; equal minima at 3 and 67 (one lane, two trips) and at 64 and 1 (two lanes).
  k_memory_insert                     float4 copies (len 4, 1024, aligned), scalar ones (len 5, 1023; src or dst one float off), len 262148 =
                                      65537 float4: past one trip of 256 blocks.
  k_filter_wgrad                      C = 1, 5, 17: channel tails of the 4-channel waves, C = 5: waves with cbase >= C leave after the barrier; parts
                                      beyond the pixels (hw = 9, parts = 8: per = 2, parts 5..7 empty) written as zeros; 126 x 126: 64 KB of LDS.
  k_filter_igrad                      both layouts; 62 x 63 x 17 = 66402 elements > 64 blocks x 1024: the grid-stride trip.
  frtm_filter_scores_pitched          the row form (N = 4, w = 64), the 16-pixel form, the 64-pixel form (505 x 65: 513 blocks), and w = 64 with
                                      N = 3, which the pixel form serves; out_pitch = h w + 7.
  k_merge_masks / _any                K = 2, 3, 16 / 17, 20; one pixel, 255, 70000 (a second grid-stride trip needs > 262144; the frames index).

No floor above the plain gate was needed, and no fault was found: nothing in csrc/target_model.hip changed with this module.  No test here
asserts a time.  The module (315 tests) ran in 8.6 to 8.8 s on an MI355X.  Largest RATIO (hip error / torch32 error) per kernel; ratios above 4 passed on
the 1e-6 floor of max|ref|:
    k_pixel_weights_map 1.00   next_slot_step 1.52   k_filter_wgrad 1.85   k_filter_wgrad<stencil> 1.63   k_filter_igrad 4.73 (5.6e-7 on values up
    to 4.1)   frtm_filter_scores_pitched 2.08   k_merge_masks 2.48   k_merge_masks_any 2.07
    k_normal_build, per tap plane 0..8: 3.53  1.34  2.30  4.00  1.10  4.00  3.53  1.34  2.30, c 2.22.  The 4.00 is 64 x 64 -> 2 x 2 with 10 pixels
    (wf = 0.1 x 4096 / 10 = 41): 4 ulp against 1 ulp of the fp32 leg on values up to 142, inside the 1e-6 floor as well (6.1e-5 against 1.4e-4).
Inserts, the transpose, the guarded copy, the counts, slots and state words are compared exactly.
"""
import pytest
import torch

import _solver_refs as S
import _target_refs as R
from test_solver_kernels_gpu import DEV, GUARD, NAN, _Buf, _bits, _call, _check, _d, _gen, _legs, _randn, _uniform

pytestmark = pytest.mark.gpu
SENT = -0x5A5A5A5B                      # guard and "not written" value of integer buffers


def _f32(x):
    """x as the fp32 value a kernel is handed."""
    return float(torch.tensor(x, dtype=torch.float32))


class _IntBuf:
    """_Buf for int32 words: SENT-filled (an output) or holding `init`, between two guard bands of SENT."""

    def __init__(self, n=None, init=None):
        if init is not None:
            init = torch.as_tensor(init, dtype=torch.int32)
            n = init.numel()
        self.buf = torch.full((n + 2 * GUARD,), SENT, dtype=torch.int32, device=DEV)
        self.t = self.buf[GUARD:GUARD + n]
        if init is not None:
            self.t.copy_(init)
        self.before = self.t.clone()

    def guards(self):
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == SENT).all()), 'write below the buffer'
        assert bool((self.buf[GUARD + self.t.numel():] == SENT).all()), 'write above the buffer'

    def done(self):
        self.guards()
        assert not bool((self.t == SENT).any()), 'output word not written'
        return self.t.tolist()

    def same(self):
        self.guards()
        assert torch.equal(self.t, self.before), 'a word that the launch must not write has changed'
        return self.t.tolist()


def _ints(v):
    return torch.as_tensor(v, dtype=torch.int32).to(DEV)


def _slots_written(buf, written):
    """buf.t (cap, ...): the guards intact, every word of the slots in `written` written, every other slot bit for bit as before."""
    buf.guards()
    for s in range(buf.t.shape[0]):
        if s in written:
            assert not bool(torch.isnan(buf.t[s]).any()), 'output element of slot %d not written' % s
        else:
            assert torch.equal(_bits(buf.t[s]), _bits(buf.before[s])), 'slot %d, which the launch must not write, has changed' % s


# ---------------------------------------------------------------------------------------------------------------------------------
# pixel weights
# ---------------------------------------------------------------------------------------------------------------------------------
def _pw_counts(HW, tf):
    if HW == 1:
        return [0, 1]
    want = [0, 9, 10, int(0.5 * tf * HW), int((tf + 0.5 * (1 - tf)) * HW)]
    return sorted(set(c for c in want if c < HW))


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('H,W', [(1, 1), (3, 5), (7, 9), (363, 362)])
def test_pixel_weights(H, W, n):
    HW = H * W
    tf = _f32(R.boundary_tf(HW))
    counts = _pw_counts(HW, tf)
    groups = [[c] for c in counts] if n == 1 else [[counts[(i + j) % len(counts)] for j in range(3)] for i in range(len(counts))]
    for grp in groups:
        y = torch.stack([R.labels_with_count(H, W, c, 100 + k) for k, c in enumerate(grp)])
        r64, r32 = _legs(lambda y_: R.pixel_weights(y_, tf), y)
        assert bool(torch.isfinite(r64).all())
        outs = []
        for u8 in (1, 0):
            lab = _d(y.to(torch.uint8) if u8 else y)
            out, scratch = _Buf(n, H, W), _Buf(n * R.PX_PARTS)
            _call('frtm_pixel_weights', lab, u8, n, H, W, tf, out.t, scratch.t)
            _check('k_pixel_weights_map', '%dx%d counts %s u8 %d' % (H, W, grp, u8), out.done(), r64, r32)
            parts = scratch.done().view(n, R.PX_PARTS)            # every part of every sample, the empty ones as zeros
            assert parts.sum(1).tolist() == [float(c) for c in grp]
            outs.append(out.t.clone())
            ones = _Buf(n, H, W)
            _call('frtm_pixel_weights', lab, u8, n, H, W, -1.0, ones.t, scratch.t)
            assert torch.equal(_bits(ones.done()), _bits(torch.ones(n, H, W, device=DEV)))
        assert torch.equal(_bits(outs[0]), _bits(outs[1])), 'u8 and float labels give different bits'


@pytest.mark.parametrize('H,W', [(3, 5), (7, 9)])
def test_pixel_weights_all_foreground(H, W):
    """Sample 0 is all foreground: af = 1, wb = 0 / 0, and so is the definition's: the same positions are non-finite, nothing else is claimed."""
    tf = _f32(0.25)
    y = torch.stack([torch.ones(H, W), R.labels_with_count(H, W, 12, 5)])
    r64, r32 = _legs(lambda y_: R.pixel_weights(y_, tf), y)
    assert not bool(torch.isfinite(r64[0]).any()) and bool(torch.isfinite(r64[1]).all())
    out, scratch = _Buf(init=torch.full((2, H, W), 7.0)), _Buf(2 * R.PX_PARTS)
    _call('frtm_pixel_weights', _d(y), 0, 2, H, W, tf, out.t, scratch.t)
    out.guards()
    assert torch.equal(torch.isfinite(out.t).cpu(), torch.isfinite(r64))
    assert not bool((out.t == 7.0).any())
    _check('k_pixel_weights_map', '%dx%d beside an all-foreground sample' % (H, W), out.t[1], r64[1], r32[1])


# ---------------------------------------------------------------------------------------------------------------------------------
# normal equations
# ---------------------------------------------------------------------------------------------------------------------------------
NORMAL_SHAPES = [(8, 8, 8, 8), (12, 40, 1, 5), (40, 12, 5, 1), (37, 53, 5, 7), (50, 120, 3, 3), (90, 20, 3, 2), (64, 64, 2, 2), (9, 10, 8, 9)]
CAP = 5


def _normal_call(lab, u8, pw, n, H, W, h, w, tf, slot_dev, slot_host, px):
    B, c, scratch = _Buf(CAP, 9, h, w), _Buf(CAP, h, w), _Buf(CAP * R.PX_PARTS)
    _call('frtm_normal_build', lab, u8, pw, n, H, W, h, w, tf, slot_dev, slot_host, B.t, c.t, scratch.t, px)
    return B, c


def _check_normals(case, B, c, slot, n, r64, r32):
    """Slots slot .. slot + n - 1 of B and c against (B, c) of the definition, every tap plane on its own; the other slots untouched."""
    written = set(range(slot, slot + n))
    _slots_written(B, written), _slots_written(c, written)
    for k in range(9):
        _check('k_normal_build', 'tap %d %s' % (k, case), B.t[slot:slot + n, k], r64[0][:, k], r32[0][:, k])
    _check('k_normal_build', 'c %s' % case, c.t[slot:slot + n], r64[1], r32[1])


def _soft_labels(g, n, H, W):
    """Soft labels: about half, about 30 % and a handful of the pixels above 0.5."""
    soft = torch.rand(n, H, W, generator=g)
    soft[1] = (soft[1] > 0.7).float() * soft[1]
    soft[2].view(-1)[3:] *= 0.4
    return soft


@pytest.mark.parametrize('H,W,h,w', NORMAL_SHAPES)
def test_normal_build(H, W, h, w):
    g = _gen(H, W, h, w, 40)
    n, tf = 3, _f32(0.5)
    soft = _soft_labels(g, n, H, W)
    assert int((soft[2] > 0.5).sum()) < 10 <= int((soft[1] > 0.5).sum()) < 0.45 * H * W
    case = '%dx%d->%dx%d' % (H, W, h, w)
    # float soft labels, hinge weights, slot_host = 2
    r64, r32 = _legs(lambda l_: R.normals(l_, None, None, h, w, tf), soft)
    B, c = _normal_call(_d(soft), 0, None, n, H, W, h, w, tf, None, 2, None)
    _check_normals('soft hinge ' + case, B, c, 2, n, r64, r32)
    # ... the counts handed in: the same bits
    cnt = _ints((soft > 0.5).sum(dim=(1, 2)))
    B1, c1 = _normal_call(_d(soft), 0, None, n, H, W, h, w, tf, None, 2, cnt)
    _slots_written(B1, {2, 3, 4}), _slots_written(c1, {2, 3, 4})
    assert torch.equal(_bits(B1.t), _bits(B.t)) and torch.equal(_bits(c1.t), _bits(c.t))
    # u8 labels with explicit pixel weights, slot_host = 0
    lab8 = (soft > 0.5).to(torch.uint8)
    pwx = torch.rand(n, H, W, generator=g) + 0.5
    r64, r32 = _legs(lambda l_, p_: R.normals(l_, p_, None, h, w, tf), lab8.float(), pwx)
    B, c = _normal_call(_d(lab8), 1, _d(pwx), n, H, W, h, w, tf, None, 0, None)
    _check_normals('u8 pw ' + case, B, c, 0, n, r64, r32)


@pytest.mark.parametrize('H,W,h,w', NORMAL_SHAPES)
def test_normal_build_counts_nine_and_ten(H, W, h, w):
    """Labels of exactly 9 and exactly 10 pixels (value 0.9) on both sides of the `px < 10` rule: summed inside, handed in (the same bits), and
    handed in the other way round (the definition with those counts: the count is read, not recomputed)."""
    tf = _f32(R.boundary_tf(H * W))
    lab = torch.stack([R.labels_with_count(H, W, 9, 1), R.labels_with_count(H, W, 10, 2)]) * 0.9
    case = '%dx%d->%dx%d' % (H, W, h, w)
    r64, r32 = _legs(lambda l_: R.normals(l_, None, None, h, w, tf), lab)
    B, c = _normal_call(_d(lab), 0, None, 2, H, W, h, w, tf, None, 2, None)
    _check_normals('9 and 10 px ' + case, B, c, 2, 2, r64, r32)
    B1, c1 = _normal_call(_d(lab), 0, None, 2, H, W, h, w, tf, None, 2, _ints([9, 10]))
    assert torch.equal(_bits(B1.t), _bits(B.t)) and torch.equal(_bits(c1.t), _bits(c.t))
    r64, r32 = _legs(lambda l_, p_: R.normals(l_, None, p_, h, w, tf), lab, torch.tensor([10.0, 9.0]))
    B2, c2 = _normal_call(_d(lab), 0, None, 2, H, W, h, w, tf, None, 2, _ints([10, 9]))
    _check_normals('counts 10 and 9 handed in ' + case, B2, c2, 2, 2, r64, r32)
    assert not torch.equal(_bits(B2.t[2:4]), _bits(B.t[2:4]))


@pytest.mark.parametrize('H,W,h,w', [(37, 53, 5, 7), (50, 120, 3, 3)])
def test_normal_build_device_slot(H, W, h, w):
    g = _gen(H, W, h, w, 41)
    tf = _f32(0.5)
    soft = _soft_labels(g, 3, H, W)[:1].contiguous()
    B0, c0 = _normal_call(_d(soft), 0, None, 1, H, W, h, w, tf, None, 3, None)
    _slots_written(B0, {3}), _slots_written(c0, {3})
    B, c = _normal_call(_d(soft), 0, None, 1, H, W, h, w, tf, _ints([3]), 0, None)
    _slots_written(B, {3}), _slots_written(c, {3})
    assert torch.equal(_bits(B.t), _bits(B0.t)) and torch.equal(_bits(c.t), _bits(c0.t))
    B, c = _normal_call(_d(soft), 0, None, 1, H, W, h, w, tf, _ints([-1]), 0, None)
    B.same(), c.same()


# ---------------------------------------------------------------------------------------------------------------------------------
# sample weights and slots
# ---------------------------------------------------------------------------------------------------------------------------------
def _next_slot(sw, cap, lr, num_zero, state, count, min_count):
    """One frtm_memory_next_slot launch on (sw _Buf, state _IntBuf)."""
    cnt = None if count is None else _ints([count])
    _call('frtm_memory_next_slot', sw.t, cap, lr, num_zero, state.t, cnt, min_count)
    torch.cuda.synchronize()


def _check_slot(case, sw0, cap, lr, num_zero, state0, count, min_count):
    sw, state = _Buf(init=sw0), _IntBuf(init=state0)
    _next_slot(sw, cap, lr, num_zero, state, count, min_count)
    (w64, st64, r64), (w32, st32, r32) = _legs(lambda s_: R.next_slot(s_, lr, num_zero, state0, count, min_count), sw0)
    assert st64 == st32 and r64 == r32
    assert state.done() == st64, (case, state.t.tolist(), st64)
    if r64 < 0:
        sw.same()
    else:
        _check('next_slot_step', case, sw.done(), w64, w32)
    return r64


@pytest.mark.parametrize('cap', [5, 64, 65, 130])
def test_memory_next_slot_branches(cap):
    g = _gen(cap, 50)
    sw0 = _uniform(g, 0.5, 1.5, cap)
    sw0 = sw0 / sw0.sum()
    lr = R.LR
    lo = int(sw0.argmin())
    prev = (lo + 2) % cap
    assert _check_slot('cap %d empty memory' % cap, sw0, cap, lr, 1, [-1, -1, 0, 0], None, 10) == 0
    assert _check_slot('cap %d lr 1' % cap, sw0, cap, 1.0, 0, [prev, prev, 4, 1], None, 10) == 0
    assert _check_slot('cap %d first replacement' % cap, sw0, cap, lr, 0, [-1, -1, 0, 0], None, 10) == lo
    assert _check_slot('cap %d later replacement' % cap, sw0, cap, lr, 0, [prev, prev, 4, 1], None, 10) == lo
    assert _check_slot('cap %d guarded, count < min' % cap, sw0, cap, lr, 0, [prev, prev, 4, 1], 9, 10) == -1
    assert _check_slot('cap %d guarded, count = min' % cap, sw0, cap, lr, 0, [prev, prev, 4, 1], 10, 10) == lo
    assert _check_slot('cap %d guarded, empty memory, count < min' % cap, sw0, cap, lr, 1, [-1, -1, 0, 0], 0, 10) == -1


@pytest.mark.parametrize('a,b', [(3, 67), (64, 1)])
def test_memory_next_slot_ties(a, b):
    """Equal minima at a and b of 130 weights: 3 and 67 meet in one lane (first and second trip), 64 and 1 in the butterfly.  The lowest wins."""
    cap = 130
    g = _gen(a, b, 51)
    sw0 = _uniform(g, 0.5, 1.5, cap)
    sw0[a] = sw0[b] = 0.25
    sw0 = sw0 / sw0.sum()
    assert float(sw0[a]) == float(sw0[b]) == float(sw0.min())
    for state0 in ([-1, -1, 0, 0], [7, 7, 2, 0]):
        assert _check_slot('tie %d / %d prev %d' % (a, b, state0[0]), sw0, cap, R.LR, 0, state0, None, 10) == min(a, b)


def test_memory_next_slot_trace():
    """40 calls on one memory of 6 slots from empty, every third frame but the first below min_count, against window()."""
    cap, lr = 6, R.LR
    counts = [5 if (f % 3 == 0 and f) else 30 for f in range(40)]
    sw, state = _Buf(init=torch.zeros(cap)), _IntBuf(init=[-1, -1, 0, 0])
    w64, st64, w32, st32 = torch.zeros(cap, dtype=torch.float64), [-1, -1, 0, 0], torch.zeros(cap, device=DEV), [-1, -1, 0, 0]
    for f, cnt in enumerate(counts):
        nz = int(f == 0)
        _next_slot(sw, cap, lr, nz, state, cnt, 10)
        w64, st64, r64 = R.next_slot(w64, lr, nz, st64, cnt, 10)
        w32, st32, r32 = R.next_slot(w32, lr, nz, st32, cnt, 10)
        assert state.done() == st64 == st32, (f, state.t.tolist(), st64, st32)
        _check('next_slot_step', 'trace step %d' % f, sw.done(), w64, w32)
    _, st_w, slots = R.window(torch.zeros(cap, dtype=torch.float64), lr, 1, [-1, -1, 0, 0], counts, 10)
    assert st_w == st64 and st64[2] == 27 and st64[3] == 13 and len(set(s for s in slots if s >= 0)) == cap


# ---------------------------------------------------------------------------------------------------------------------------------
# inserts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ln,src_off,dst_off', [(4, 0, 0), (1024, 0, 0), (5, 0, 0), (1023, 0, 0), (1024, 1, 0), (1024, 0, 1), (262148, 0, 0)])
def test_memory_insert(ln, src_off, dst_off):
    cap = 3
    g = _gen(ln, src_off, dst_off, 60)
    src = _Buf(init=_randn(g, ln + src_off))
    dst = _Buf(init=_randn(g, cap * ln + dst_off))
    s, d = src.t[src_off:], dst.t[dst_off:]
    assert (s.data_ptr() % 16 == 0) == (src_off == 0) and (d.data_ptr() % 16 == 0) == (dst_off == 0)
    _call('frtm_memory_insert', s, d, ln, _ints([-1]))
    dst.same(), src.same()
    _call('frtm_memory_insert', s, d, ln, _ints([1]))
    src.same()
    dst.guards()
    want = dst.before.clone()
    want[dst_off + ln:dst_off + 2 * ln] = s
    assert torch.equal(_bits(dst.t), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------------------
# window update
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('start', ['repeat', 'distinct', 'empty'])
def test_memory_update_window(start):
    """W = 5 frames into 3 slots, frames 1 and 3 below min_count, labels 7 floats further apart than they are long, counts in every second
    word (the words between say the opposite: a stride that is not read changes the slots) == five frame-by-frame updates, bit for bit.
    repeat: slot 2 is taken by frames 0, 2 and 4 and holds frame 4; distinct: 2, 1, 0; empty: an empty memory, 0, 1, 2."""
    Wn, cap, C, h, w, H, Wd, tf, lr = 5, 3, 2, 3, 4, 12, 18, _f32(0.25), R.LR
    ln, stride = C * h * w, H * Wd + 7
    g = _gen(70)
    feats = _randn(g, Wn, ln)
    labels = torch.full((Wn, stride), NAN)
    px = [40, 3, 55, 7, 25]
    for f in range(Wn):
        labels[f, :H * Wd] = R.labels_with_count(H, Wd, px[f], 70 + f).view(-1) * 0.8 + torch.rand(H * Wd, generator=g) * 0.1
    counts = torch.tensor([[px[f], 0 if px[f] >= 10 else 1000] for f in range(Wn)], dtype=torch.int32)
    sw0 = torch.zeros(cap) if start == 'empty' else torch.tensor([0.5, 0.3, 0.2])
    state0 = [0, 0, 4, 1] if start == 'distinct' else [-1, -1, 0, 0]
    nz = int(start == 'empty')
    want_slots = {'repeat': [2, -1, 2, -1, 2], 'distinct': [2, -1, 1, -1, 0], 'empty': [0, -1, 1, -1, 2]}[start]
    assert R.window(sw0.double(), lr, nz, state0, px, 10)[2] == want_slots
    fd, ld, cd = _d(feats), _d(labels), _d(counts)

    def buffers():
        return (_Buf(init=sw0), _IntBuf(init=state0), _Buf(cap, ln), _Buf(cap, 9, h, w), _Buf(cap, h, w), _Buf(8 * R.PX_PARTS))
    # frame by frame
    sw1, st1, smp1, B1, c1, scr1 = buffers()
    seq = []
    for f in range(Wn):
        cnt_f = cd.data_ptr() + 8 * f
        _call('frtm_memory_next_slot', sw1.t, cap, lr, nz, st1.t, cnt_f, 10)
        slot_ptr = st1.t.data_ptr() + 4
        _call('frtm_memory_insert', fd[f], smp1.t, ln, slot_ptr)
        _call('frtm_normal_build', ld.data_ptr() + 4 * f * stride, 0, None, 1, H, Wd, h, w, tf, slot_ptr, 0, B1.t, c1.t, scr1.t, cnt_f)
        torch.cuda.synchronize()
        seq.append(int(st1.t[1]))
        if seq[-1] >= 0:
            nz = 0
    assert seq == want_slots
    # one call
    sw2, st2, smp2, B2, c2, scr2 = buffers()
    slots = _IntBuf(Wn)
    _call('frtm_memory_update_window', sw2.t, cap, lr, int(start == 'empty'), st2.t, cd, 2, 10, Wn, slots.t, fd, smp2.t, ln, ld, stride, H, Wd, h, w, tf,
          B2.t, c2.t, scr2.t)
    assert slots.done() == seq
    assert st2.done() == st1.done()
    taken = set(s for s in seq if s >= 0)
    for one, two in ((smp1, smp2), (B1, B2), (c1, c2)):
        _slots_written(one, taken), _slots_written(two, taken)
        assert torch.equal(_bits(one.t), _bits(two.t))
    assert torch.equal(_bits(sw1.done()), _bits(sw2.done()))
    last = {s: f for f, s in enumerate(seq) if s >= 0}            # a slot taken twice holds the later frame
    for s, f in last.items():
        assert torch.equal(_bits(smp2.t[s]), _bits(fd[f]))
        lab_f = labels[f:f + 1, :H * Wd].reshape(1, H, Wd)
        r64, r32 = _legs(lambda l_, p_: R.normals(l_, None, p_, h, w, tf), lab_f, torch.tensor([float(px[f])]))
        for k in range(9):
            _check('k_normal_build', 'window %s slot %d tap %d' % (start, s, k), B2.t[s:s + 1, k], r64[0][:, k], r32[0][:, k])
        _check('k_normal_build', 'window %s slot %d c' % (start, s), c2.t[s:s + 1], r64[1], r32[1])
    w64, w32 = R.window(sw0.double(), lr, int(start == 'empty'), state0, px, 10)[0], R.window(_d(sw0), lr, int(start == 'empty'), state0, px, 10)[0]
    _check('next_slot_step', 'window %s' % start, sw2.t, w64, w32)


# ---------------------------------------------------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------------------------------------------------
GRAD_MAPS = [(1, 1), (3, 3), (7, 9), (5, 65), (17, 31)]


def _wgrad_case(N, C, h, w, parts):
    g = _gen(N, C, h, w, 80)
    X, t = _randn(g, N, C, h, w), _randn(g, N, h, w)
    partial = _Buf(N * parts, C * 9)
    _call('frtm_filter_wgrad', _d(X), _d(t), N, C, h, w, parts, partial.t)
    r64, r32 = _legs(S.filter_wgrad, X, t)
    slabs = partial.done().view(N, parts, C * 9)                  # every slab word, those of the empty parts included
    per = -(-h * w // parts)
    for p in range(parts):
        if p * per >= h * w:
            assert bool((slabs[:, p] == 0).all()), 'the slab of an empty part is not zero'
    _check('k_filter_wgrad', 'N%d C%d %dx%d parts %d' % (N, C, h, w, parts), slabs.double().sum(1), r64, r32)


@pytest.mark.parametrize('N', [1, 3])
@pytest.mark.parametrize('parts', [1, 3, 8, 64])
@pytest.mark.parametrize('h,w', GRAD_MAPS)
@pytest.mark.parametrize('C', [1, 5, 16, 17])
def test_filter_wgrad(C, h, w, parts, N):
    _wgrad_case(N, C, h, w, parts)


def test_filter_wgrad_largest_tile():
    assert 128 * 128 * 4 == 64 * 1024
    _wgrad_case(1, 2, 126, 126, 1)


@pytest.mark.parametrize('with_c', [False, True])
@pytest.mark.parametrize('h,w', GRAD_MAPS + [(88, 88)])
@pytest.mark.parametrize('C', [1, 5, 16, 17])
def test_filter_wgrad_stencil(C, h, w, with_c):
    if (h, w) == (88, 88):
        assert 2 * 90 * 90 * 4 <= 64 * 1024 < 2 * 91 * 91 * 4
        if C != 5:
            return                                                # the largest tile once
    N = 2
    g = _gen(C, h, w, with_c, 81)
    X, s = _randn(g, N, C, h, w), _randn(g, N, h, w)
    B, c, sw = _randn(g, N, 9, h, w), (_randn(g, N, h, w) if with_c else None), _uniform(g, 0.1, 1.0, N)
    partial = _Buf(N, C * 9)
    _call('frtm_filter_wgrad_stencil', _d(X), _d(s), _d(B), _d(c), _d(sw), N, C, h, w, partial.t)
    r64, r32 = _legs(lambda X_, s_, B_, c_, sw_: S.filter_wgrad(X_, S.stencil(B_, c_, sw_, s_)), X, s, B, c, sw)
    _check('k_filter_wgrad<stencil>', 'C%d %dx%d c %d' % (C, h, w, with_c), partial.done(), r64, r32)


# ---------------------------------------------------------------------------------------------------------------------------------
# input gradient
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,h,w', [(C, h, w) for C in (1, 5, 17) for h, w in GRAD_MAPS] + [(17, 62, 63)])
def test_filter_igrad(C, h, w):
    N = 2
    g = _gen(C, h, w, 82)
    t, f = _randn(g, N, h, w), _randn(g, C, 9) * 0.3
    r64, r32 = _legs(S.filter_igrad, t, f)                        # pix-major (N, hw, C)
    Dp, Dc = _Buf(N, h * w, C), _Buf(N, C, h * w)
    _call('frtm_filter_igrad', _d(t), _d(f), N, C, h, w, Dp.t, 1)
    _call('frtm_filter_igrad', _d(t), _d(f), N, C, h, w, Dc.t, 0)
    case = 'C%d %dx%d' % (C, h, w)
    _check('k_filter_igrad', 'pix-major ' + case, Dp.done(), r64, r32)
    _check('k_filter_igrad', 'channel-major ' + case, Dc.done(), r64.transpose(1, 2), r32.transpose(1, 2))
    assert torch.equal(_bits(Dp.t.transpose(1, 2).contiguous()), _bits(Dc.t))


# ---------------------------------------------------------------------------------------------------------------------------------
# pitched scores
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,C,h,w', [(4, 17, 5, 64), (1, 5, 7, 9), (1, 3, 505, 65), (3, 5, 5, 64)])
def test_filter_scores_pitched(N, C, h, w):
    hw, pitch = h * w, h * w + 7
    g = _gen(N, C, h, w, 83)
    X, f = _randn(g, N, C, h, w), _randn(g, C, 9) * 0.3
    r64, r32 = _legs(S.conv3x3, X, f)
    case = 'N%d C%d %dx%d' % (N, C, h, w)
    out = _Buf(N, pitch)
    _call('frtm_filter_scores_pitched', _d(X), _d(f), N, C, h, w, out.t, pitch, 0)
    out.guards()
    assert torch.equal(_bits(out.t[:, hw:]), _bits(out.before[:, hw:])), 'a word between two maps was written'
    assert not bool(torch.isnan(out.t[:, :hw]).any()), 'output element not written'
    _check('frtm_filter_scores_pitched', case, out.t[:, :hw].reshape(N, h, w), r64, r32)
    start = torch.full((N, pitch), NAN)
    start[:, :hw] = _randn(g, N, hw)
    acc = _Buf(init=start)
    _call('frtm_filter_scores_pitched', _d(X), _d(f), N, C, h, w, acc.t, pitch, 1)
    acc.guards()
    assert torch.equal(_bits(acc.t[:, hw:]), _bits(acc.before[:, hw:])), 'a word between two maps was written'
    a64, a32 = start[:, :hw].reshape(N, h, w).double() + r64, _d(start[:, :hw].reshape(N, h, w)) + r32
    _check('frtm_filter_scores_pitched', 'accumulate ' + case, acc.t[:, :hw].reshape(N, h, w), a64, a32)


# ---------------------------------------------------------------------------------------------------------------------------------
# transpose, guarded copy
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,cols', [(1, 1), (1, 70), (70, 1), (33, 31), (32, 64), (37, 5)])
def test_transpose2d(rows, cols):
    x = _randn(_gen(rows, cols, 84), rows, cols)
    out = _Buf(cols, rows)
    _call('frtm_transpose2d', _d(x), rows, cols, out.t)
    assert torch.equal(_bits(out.done()), _bits(_d(x.t().contiguous())))


@pytest.mark.parametrize('n', [1, 255, 70000])
def test_guarded_copy(n):
    g = _gen(n, 85)
    src0, dst0 = _randn(g, n), _randn(g, n)
    src = _Buf(init=src0)

    def run(guard, guard_min, mode, count, with_stats=True):
        dst, stats = _Buf(init=dst0), _IntBuf(init=[7, 11, 13, 17])
        _call('frtm_guarded_copy', dst.t, src.t, n, None if guard is None else _ints([guard]), guard_min, mode, stats.t if with_stats else None, count)
        src.same()
        return dst, stats

    def copied(dst):
        dst.guards()
        assert torch.equal(_bits(dst.t), _bits(src.t))
    for count in (0, 1):
        dst, stats = run(None, 10, 0, count)                      # mode 0: a copy, whatever the guard; nothing is counted
        copied(dst), stats.same()
        dst, stats = run(50, 10, 0, count)
        copied(dst), stats.same()
        dst, stats = run(9, 10, 1, count)                         # below the minimum: roll back
        copied(dst)
        assert stats.done() == [7, 11 + count, 13, 17]
        dst, stats = run(10, 10, 1, count)                        # equal to it: the update stands
        dst.same()
        assert stats.done() == [7 + count, 11, 13, 17]
    dst, _ = run(9, 10, 1, 1, with_stats=False)
    copied(dst)
    dst, stats = _Buf(init=dst0), _IntBuf(init=[7, 11, 13, 17])
    with pytest.raises(RuntimeError, match='frtm_guarded_copy: bad argument'):                # mode 1 with a null guard is refused on the host
        _call('frtm_guarded_copy', dst.t, src.t, n, None, 10, 1, stats.t, 1)
    dst.same(), stats.same()


# ---------------------------------------------------------------------------------------------------------------------------------
# mask merge, count
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,HW,frames', R.MERGE_CASES)
def test_merge_masks(K, HW, frames):
    """Plane 0 of the input is never read: it holds NaN on entry, so done() shows that the launch wrote it."""
    m, ties = R.merge_input(K, HW, frames)
    m[:, 0] = NAN
    (o64, a64, margin), (o32, _, _) = _legs(R.merge, m)
    entries = ['frtm_merge_masks_frames'] + (['frtm_merge_masks'] if frames == 1 else [])
    for entry in entries:
        buf = _Buf(init=m)
        if entry == 'frtm_merge_masks':
            _call(entry, buf.t, K, HW)
        else:
            _call(entry, buf.t, frames, K, HW)
        out = buf.done().cpu()
        assert bool(((out != 0).sum(1) == 1).all()), 'more or fewer than one plane of a pixel is non-zero'
        case = 'K%d HW%d frames %d' % (K, HW, frames)
        _check('k_merge_masks' if K <= R.MERGE_MAX else 'k_merge_masks_any', case, out.amax(1), o64.amax(1), o32.amax(1))
        checked = R.merge_checked(margin)
        assert torch.equal(out.argmax(1)[checked], a64[checked]), 'another plane wins where the margin decides'
        for px, plane in ties.items():
            assert bool(checked[:, px].all()) and bool((out[:, plane, px] > 0).all())


def test_count_above_threshold_and_alignment():
    """Values equal to thr are not counted.  HW = 4099 from an address 4 bytes past a 16-byte boundary: plane 0 is 4-byte but not 16-byte
    aligned (the scalar loads), plane 1 starts 4 + 4 * 4099 = 16400 bytes on, 16-byte aligned (float4 loads and a tail of three)."""
    n, HW, thr = 2, 4099, _f32(0.37)
    g = _gen(86)
    m = torch.rand(n, HW, generator=g)
    m[0, ::5] = thr
    m[1, 1::3] = thr
    buf = _Buf(init=torch.cat([torch.zeros(1), m.reshape(-1)]))
    planes = buf.t[1:]
    assert planes.data_ptr() % 16 == 4 and (planes.data_ptr() + 4 * HW) % 16 == 0 and HW % 4 == 3
    cnt = _IntBuf(n)
    _call('frtm_count_above', planes, n, HW, thr, cnt.t)
    assert cnt.done() == (m > thr).sum(1).tolist()
    buf.same()
    aligned, cnt = _Buf(init=m[0]), _IntBuf(1)
    _call('frtm_count_above', aligned.t, 1, HW, thr, cnt.t)
    assert cnt.done() == [int((m[0] > thr).sum())]


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals: each is refused on the host before any launch and leaves its outputs untouched
# ---------------------------------------------------------------------------------------------------------------------------------
def _z(*shape):
    return torch.zeros(*shape, device=DEV)


def test_refusals():
    out, scratch = _Buf(2, 3, 4), _Buf(2 * R.PX_PARTS)
    with pytest.raises(RuntimeError, match='frtm_pixel_weights: bad argument'):
        _call('frtm_pixel_weights', None, 0, 2, 3, 4, 0.1, out.t, scratch.t)
    with pytest.raises(RuntimeError, match='frtm_pixel_weights: bad argument'):
        _call('frtm_pixel_weights', _z(2, 3, 4), 0, 0, 3, 4, 0.1, out.t, scratch.t)
    out.same(), scratch.same()

    B, c = _Buf(2, 9, 3, 4), _Buf(2, 3, 4)
    with pytest.raises(RuntimeError, match='frtm_normal_build: bad argument'):
        _call('frtm_normal_build', None, 0, None, 1, 12, 16, 3, 4, 0.1, None, 0, B.t, c.t, scratch.t, None)
    with pytest.raises(RuntimeError, match='frtm_normal_build: bad argument'):
        _call('frtm_normal_build', _z(1, 12, 16), 0, None, 1, 12, 16, 3, 4, 0.1, None, 0, B.t, c.t, None, None)
    with pytest.raises(RuntimeError, match='frtm_normal_build: needs H>=h, W>=w'):
        _call('frtm_normal_build', _z(1, 2, 16), 0, None, 1, 2, 16, 3, 4, 0.1, None, 0, B.t, c.t, scratch.t, None)
    with pytest.raises(RuntimeError, match='frtm_normal_build: needs H>=h, W>=w'):
        _call('frtm_normal_build', _z(1, 12, 3), 0, None, 1, 12, 3, 3, 4, 0.1, None, 0, B.t, c.t, scratch.t, None)
    B.same(), c.same(), scratch.same()

    sw, state, slots, smp = _Buf(init=torch.tensor([0.5, 0.5])), _IntBuf(init=[-1, -1, 0, 0]), _IntBuf(2), _Buf(2, 24)
    def win(counts, H):
        _call('frtm_memory_update_window', sw.t, 2, 0.1, 0, state.t, counts, 1, 10, 2, slots.t, _z(2, 24), smp.t, 24, _z(2, 12 * 16), 12 * 16, H, 16,
              3, 4, 0.1, B.t, c.t, scratch.t)
    with pytest.raises(RuntimeError, match='frtm_memory_update_window: bad argument'):
        win(None, 12)
    with pytest.raises(RuntimeError, match='frtm_memory_update_window: needs H>=h, W>=w'):
        win(_ints([20, 20]), 2)
    with pytest.raises(RuntimeError, match='frtm_memory_next_slot: bad argument'):
        _call('frtm_memory_next_slot', None, 2, 0.1, 0, state.t, None, 10)
    with pytest.raises(RuntimeError, match='frtm_memory_next_slot: bad argument'):
        _call('frtm_memory_next_slot', sw.t, 0, 0.1, 0, state.t, None, 10)
    with pytest.raises(RuntimeError, match='frtm_memory_insert: bad argument'):
        _call('frtm_memory_insert', _z(24), smp.t, 24, None)
    with pytest.raises(RuntimeError, match='frtm_memory_insert: bad argument'):
        _call('frtm_memory_insert', _z(24), smp.t, 0, _ints([0]))
    sw.same(), state.same(), slots.same(), smp.same(), B.same(), c.same()

    part = _Buf(65, 2 * 9)
    for parts in (0, 65):
        with pytest.raises(RuntimeError, match='frtm_filter_wgrad: bad argument'):
            _call('frtm_filter_wgrad', _z(1, 2, 3, 3), _z(1, 3, 3), 1, 2, 3, 3, parts, part.t)
    with pytest.raises(RuntimeError, match='frtm_filter_wgrad: bad argument'):
        _call('frtm_filter_wgrad', _z(1, 2, 3, 3), None, 1, 2, 3, 3, 1, part.t)
    assert 129 * 128 * 4 > 64 * 1024
    with pytest.raises(RuntimeError, match='frtm_filter_wgrad: feature grid 127x126 too large for the LDS tile'):
        _call('frtm_filter_wgrad', _z(1, 2, 127, 126), _z(1, 127, 126), 1, 2, 127, 126, 1, part.t)
    with pytest.raises(RuntimeError, match='frtm_filter_wgrad_stencil: bad argument'):
        _call('frtm_filter_wgrad_stencil', _z(1, 2, 3, 3), _z(1, 3, 3), None, None, _z(1), 1, 2, 3, 3, part.t)
    with pytest.raises(RuntimeError, match='frtm_filter_wgrad_stencil: feature grid 89x89 too large for the LDS tile'):
        _call('frtm_filter_wgrad_stencil', _z(1, 2, 89, 89), _z(1, 89, 89), _z(1, 9, 89, 89), None, _z(1), 1, 2, 89, 89, part.t)
    part.same()

    D = _Buf(1, 2, 127 * 126)
    with pytest.raises(RuntimeError, match='frtm_filter_igrad: bad argument'):
        _call('frtm_filter_igrad', _z(1, 3, 3), None, 1, 2, 3, 3, D.t, 0)
    for pix_major in (0, 1):
        with pytest.raises(RuntimeError, match='frtm_filter_igrad: feature grid 127x126 too large for the LDS tile'):
            _call('frtm_filter_igrad', _z(1, 127, 126), _z(2, 9), 1, 2, 127, 126, D.t, pix_major)
    D.same()

    s = _Buf(2, 70)
    with pytest.raises(RuntimeError, match='frtm_filter_scores: bad argument'):
        _call('frtm_filter_scores_pitched', _z(2, 3, 7, 9), _z(3, 9), 2, 3, 7, 9, s.t, 62, 0)
    with pytest.raises(RuntimeError, match='frtm_filter_scores: bad argument'):
        _call('frtm_filter_scores_pitched', _z(2, 3, 7, 9), None, 2, 3, 7, 9, s.t, 70, 0)
    with pytest.raises(RuntimeError, match='frtm_transpose2d: bad argument'):
        _call('frtm_transpose2d', None, 7, 10, s.t)
    with pytest.raises(RuntimeError, match='frtm_transpose2d: bad argument'):
        _call('frtm_transpose2d', _z(7, 10), 0, 10, s.t)
    with pytest.raises(RuntimeError, match='frtm_guarded_copy: bad argument'):
        _call('frtm_guarded_copy', s.t, _z(140), 140, _ints([3]), 10, 2, None, 0)
    with pytest.raises(RuntimeError, match='frtm_guarded_copy: bad argument'):
        _call('frtm_guarded_copy', s.t, None, 140, None, 10, 0, None, 0)
    with pytest.raises(RuntimeError, match='frtm_merge_masks: needs >= 2 mask planes, got 1'):
        _call('frtm_merge_masks', s.t, 1, 140)
    with pytest.raises(RuntimeError, match='frtm_merge_masks: needs >= 2 mask planes, got 1'):
        _call('frtm_merge_masks_frames', s.t, 2, 1, 70)
    cnt = _IntBuf(2)
    with pytest.raises(RuntimeError, match='frtm_count_above: bad argument'):
        _call('frtm_count_above', None, 2, 70, 0.5, cnt.t)
    with pytest.raises(RuntimeError, match='frtm_count_above: bad argument'):
        _call('frtm_count_above', s.t, 2, 70, 0.5, None)
    s.same(), cnt.same()
