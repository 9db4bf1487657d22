"""CPU side of the per-kernel checks of the memory and gradient half of csrc/target_model.hip: the definitions of tests/_target_refs.py are
pinned here in float64, so that a wrong definition cannot pass as a right kernel.

(a) pixel_weights equals oracle.cpu_ref.pixel_weights (float64, 1e-12) and the recording g1_pixel_weights of the reference (fp32 values: 1e-6).
(b) normals equals oracle.cpu_ref.lowres_normal -- the same sums in the oracle's fp32 taps: every tap plane rel-to-its-own-max below 1e-5 --
    with hinge weights and with explicit ones, at a non-integer ratio and at a map one cell high.
(c) next_slot equals oracle.cpu_ref.MemoryRef in float64 (1e-12, slots exact) and the 100-step slot and weight traces of g2_memory, for both
    capacities; the guarded call changes the two counters and nothing else.
(d) merge equals oracle.cpu_ref.merge_masks: float64 to 1e-12 on inputs inside the clamp bounds (the oracle clamps at 1 - 1e-7 as float64 holds
    it, the kernel and the definition at the fp32 value), and to 2e-6 of the oracle's fp32 run on clamped inputs.

The conditions tests/test_target_data_gpu.py relies on:
(e) merge cap: in every merge case the margin rule leaves at most 1 % of the pixels out of the exact winner comparison (exact ties, margin
    0, are compared, not left out: fp32 is exact there and the tie rule decides), and none where a case has one pixel.
(f) hinge boundary: at every shape and tf the GPU tests use for it, labels of 9 and of 10 foreground pixels get weights more than 1e-3 apart.
"""
import numpy as np
import pytest
import torch

import _target_refs as R

from oracle import cpu_ref as O

T = torch.from_numpy
D = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) pixel weights
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pixel_weights_equal_the_oracle_and_the_recording(golden):
    g = golden('g1_pixel_weights')
    y = T(g['masks']).to(D)
    tf = float(g['tf'])
    got = R.pixel_weights(y[:, 0], tf)
    assert float((got - O.pixel_weights(y, dict(method='hinge', tf=tf), D)[:, 0]).abs().max()) <= 1e-12
    assert float((got - T(g['weights'])[:, 0].to(D)).abs().max()) < 1e-6
    assert torch.equal(R.pixel_weights(y[:, 0], -1.0), torch.ones_like(y[:, 0]))
    counts = y.sum(dim=(1, 2, 3))
    assert bool((counts < 10).any()) and bool((counts / y[0].numel() > tf).any()) and bool(((counts >= 10) & (counts / y[0].numel() < tf)).any())


def test_hinge_rules():
    px = torch.tensor([0.0, 9.0, 10.0, 50.0, 400.0], dtype=D)
    wf, wb = R.hinge(px, 1000.0, 0.1)
    assert torch.equal(wf[:2], torch.ones(2, dtype=D)) and torch.equal(wb[:2], torch.ones(2, dtype=D))             # px < 10: af = tf
    assert abs(float(wf[2]) - 10.0) < 1e-12 and abs(float(wb[2]) - 0.9 / 0.99) < 1e-12                               # af = 0.01 < tf
    assert float(wf[4]) == 1.0 and float(wb[4]) == 1.0                                                               # af > tf: tfe = af
    wf, wb = R.hinge(torch.tensor([100.0], dtype=D), 100.0, 0.1)                                                     # all foreground: 0 / 0
    assert float(wf) == 1.0 and bool(torch.isnan(wb))
    wf, wb = R.hinge(px, 1000.0, -1.0)
    assert torch.equal(wf, torch.ones(5, dtype=D)) and torch.equal(wb, torch.ones(5, dtype=D))


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) normal equations
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,h,w', [(37, 53, 5, 7), (12, 40, 1, 5), (8, 8, 8, 8), (50, 120, 3, 3)])
def test_normals_equal_the_oracle(H, W, h, w):
    g = torch.Generator().manual_seed(H * W + h)
    n = 3
    soft = torch.rand(n, 1, H, W, generator=g)
    soft[1] = (soft[1] > 0.7).float() * soft[1]                   # 30 % foreground: below tf
    soft[2, :, 1:] = 0                                            # fewer than 10 pixels above 0.5 at most shapes
    tf = 0.5
    pw = O.pixel_weights((soft > 0.5).float(), dict(method='hinge', tf=tf))
    assert float(pw.min()) < float(pw.max())
    pwx = torch.rand(n, 1, H, W, generator=g) + 0.5
    for pw_given, pw_ref in ((None, pw), (pwx, pwx)):
        B_ref, c_ref = O.lowres_normal(pw_ref, soft, (h, w))
        B, c = R.normals(soft[:, 0].to(D), None if pw_given is None else pw_given[:, 0].to(D), None, h, w, tf)
        for k in range(9):
            if float(B_ref[:, k].abs().max()) == 0.0:             # a tap that leaves the grid (h = 1) or the identity's off-centre taps
                assert float(B[:, k].abs().max()) == 0.0, k
            else:
                assert _rel(B[:, k], B_ref[:, k].to(D)) < 1e-5, k
        assert _rel(c, c_ref.to(D)) < 1e-5
    # a count handed in replaces the sum, and only it
    cnt = (soft[:, 0] > 0.5).sum(dim=(1, 2)).to(D)
    B1, c1 = R.normals(soft[:, 0].to(D), None, cnt, h, w, tf)
    B0, c0 = R.normals(soft[:, 0].to(D), None, None, h, w, tf)
    assert torch.equal(B1, B0) and torch.equal(c1, c0)
    B2, _ = R.normals(soft[:, 0].to(D), None, torch.full((n,), 9.0, dtype=D), h, w, tf)
    assert _rel(B2[:2], B0[:2]) > 1e-3


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) sample weights and slots
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cap', [80, 8])
def test_next_slot_equals_the_oracle_and_the_recording(golden, cap):
    g = golden('g2_memory')
    lr = 0.1
    om = O.MemoryRef(cap, (1,), (1,), lr, D)
    om.initialize(torch.zeros(5, 1, dtype=D), torch.zeros(5, 1, dtype=D), torch.zeros(5, 1, dtype=D))
    sw, state = om.weights.clone(), [-1, -1, 0, 0]
    assert float((sw - T(g['w%d' % cap][0]).to(D)).abs().max()) < 1e-7
    for t in range(100):
        om.update(torch.zeros(1, dtype=D), torch.zeros(1, dtype=D), torch.zeros(1, dtype=D))
        sw, state, r = R.next_slot(sw, lr, 0, state, None, 10)
        assert r == om.prev_ind == int(g['ind%d' % cap][t]), (cap, t)
        assert state == [r, r, t + 1, 0]
        assert float((sw - om.weights).abs().max()) <= 1e-12, (cap, t)
        assert float((sw - T(g['w%d' % cap][t + 1]).to(D)).abs().max()) < 2e-7, (cap, t)
    # the same trace through window(), and the guarded call
    sw_w, st_w, slots = R.window(om.weights * 0 + T(g['w%d' % cap][0]).to(D), lr, 0, [-1, -1, 0, 0], [None] * 100, 10)
    assert slots == [int(v) for v in g['ind%d' % cap]] and st_w == [slots[-1], slots[-1], 100, 0]
    sw2, st2, r2 = R.next_slot(sw, lr, 0, state, 9, 10)
    assert r2 == -1 and torch.equal(sw2, sw) and st2 == [state[0], -1, state[2], 1]
    sw3, st3, r3 = R.next_slot(sw, lr, 0, state, 10, 10)
    assert r3 >= 0 and st3[2] == state[2] + 1 and not torch.equal(sw3, sw)


def test_next_slot_branches():
    sw = torch.tensor([0.3, 0.1, 0.4, 0.1, 0.1], dtype=D)
    for num_zero, lr in ((1, 0.1), (0, 1.0)):                     # an empty memory, lr = 1: e_0
        out, st, r = R.next_slot(sw, lr, num_zero, [3, 3, 7, 2], None, 10)
        assert r == 0 and out.tolist() == [1.0, 0.0, 0.0, 0.0, 0.0] and st == [0, 0, 8, 2]
    out, st, r = R.next_slot(sw, 0.1, 0, [-1, -1, 0, 0], None, 10)                    # first replacement; the tie goes to index 1
    want = sw / 0.9
    want[1] = 0.1
    assert r == 1 and float((out - want / want.sum()).abs().max()) <= 1e-15 and st == [1, 1, 1, 0]
    out, st, r = R.next_slot(sw, 0.1, 0, [2, 2, 4, 0], None, 10)                      # a later one
    want = sw.clone()
    want[1] = 0.4 / 0.9
    assert r == 1 and float((out - want / want.sum()).abs().max()) <= 1e-15 and st == [1, 1, 5, 0]
    # a window whose first frame fills an empty memory: the second frame no longer sees it as empty
    _, st, slots = R.window(torch.zeros(3, dtype=D), 0.1, 1, [-1, -1, 0, 0], [20, 3, 20, 20], 10)
    assert slots == [0, -1, 1, 2] and st == [2, 2, 3, 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) merge
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [2, 3, 17])
def test_merge_equals_the_oracle(K):
    g = torch.Generator().manual_seed(K)
    inside = (torch.rand(K, 300, generator=g) * 0.98 + 0.01).to(D)
    out, arg, margin = R.merge(inside)
    ref = O.merge_masks(inside.clone())
    assert float((out - ref).abs().max()) <= 1e-12
    assert torch.equal(arg, ref.argmax(0)) and float(margin.min()) > 0
    m, _ = R.merge_input(K, 255, 1)                               # clamped and planted values: against the oracle's fp32 run
    out, arg, margin = R.merge(m[0].to(D))
    ref = O.merge_masks(m[0].clone())
    ok = (margin > 1e-5) | (margin == 0)
    assert float((out - ref.to(D))[:, ok].abs().max()) < 2e-6 and torch.equal(arg[ok], ref.argmax(0)[ok]) and float(ok.float().mean()) > 0.98
    assert bool(((out != 0).sum(0) == 1).all())


def test_merge_tie_rule_and_frames():
    m = torch.tensor([[9.0, 9.0], [0.75, 0.5], [0.75, 0.25]], dtype=D)
    out, arg, margin = R.merge(m)
    assert arg.tolist() == [1, 0] and margin.tolist() == [0.0, 0.0]
    e3, e1 = float(np.exp(1.0 / 3.0 - 3.0)), float(np.exp(1.0 / 3.0 - 1.0))
    assert abs(float(out[1, 0]) - 1.0 / (2.0 + e3)) < 1e-15 and abs(float(out[0, 1]) - 1.0 / (2.0 + e1)) < 1e-15
    both = torch.stack([m, m.flip(-1)])
    outf, argf, _ = R.merge(both)
    assert torch.equal(outf[0], out) and torch.equal(outf[1], out.flip(-1)) and torch.equal(argf[1], arg.flip(-1))


# ---------------------------------------------------------------------------------------------------------------------------------
# (e), (f) the conditions of the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,HW,frames', R.MERGE_CASES)
def test_merge_cases_stay_within_the_margin_cap(K, HW, frames):
    m, ties = R.merge_input(K, HW, frames)
    out, arg, margin = R.merge(m.to(D))
    checked = R.merge_checked(margin)
    left_out = 1.0 - float(checked.double().mean())
    print('merge K %d HW %d frames %d: %.4f %% of the pixels left out' % (K, HW, frames, 100 * left_out))
    assert left_out <= (0.0 if HW == 1 else 0.01)
    for px, plane in ties.items():
        assert bool((arg[:, px] == plane).all()) and float(margin[:, px].max()) == 0.0
    if HW >= 255:                                                 # the planted 1 is clamped and wins its pixel (first among the clamped)
        assert bool((arg[:, 1] == 1).all())


BOUNDARY_SHAPES = [(3, 5), (7, 9), (363, 362), (8, 8), (12, 40), (40, 12), (37, 53), (50, 120), (90, 20), (64, 64), (9, 10)]


@pytest.mark.parametrize('H,W', BOUNDARY_SHAPES)
def test_nine_and_ten_pixels_get_different_weights(H, W):
    tf = R.boundary_tf(H * W)
    w9 = R.pixel_weights(R.labels_with_count(H, W, 9, 1)[None].to(D), tf)
    w10 = R.pixel_weights(R.labels_with_count(H, W, 10, 1)[None].to(D), tf)
    assert float(w9.min()) == 1.0 and float(w9.max()) == 1.0
    assert bool(torch.isfinite(w10).all()) and float((w10 - 1).abs().min()) > 1e-3
