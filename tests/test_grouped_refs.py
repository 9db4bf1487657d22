"""CPU side of the checks of grouped target-model scoring (csrc/target_apply_grouped.hip): the case table and the float64 definition of
tests/_grouped_refs.py are pinned here, so that a table which misses a form, or data that cannot tell a mix-up, cannot pass as a right kernel.

(a) Every form is reached.  frtm_target_apply_grouped_tiles -- the function the launcher itself chooses its kernel with -- is the literal rule
    FM = ceil(c / 32), FN = 2 from ceil(hw / 64) * G >= 256 on; through it the table reaches all eight (FM, FN) forms, every c of the row tails
    at FN = 1, and the pairs (255, 256) at 64 pixels sit on either side of the FN switch.  The table also holds the chunk counts, map sizes,
    channel groups, the pitch and the address offsets the GPU module relies on.
(b) The cases tell a mix-up apart: for every case and every pair, the float64 result computed with the neighbouring weight set, with the
    neighbouring frame, or with w1T read as [c][Cin] differs from the right one by more than 100 times the bound at some element, in the
    projected features and in the scores.  (One weight set or one frame: against a second draw.  c = 1: [Cin][1] and [1][Cin] are the same
    memory, there is no transposed reading to tell apart.)
(c) The definition is the per-pair path: Discriminator.apply of the reference (model/discriminator.py:201-205) is project, a bias-free 1x1
    convolution, then filter, a bias-free 3x3 convolution with padding 1; in float64 the two agree to 1e-12.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _grouped_refs as R


def _tiles(G, c, h, w):
    from frtm_vos_amd import _hip
    fm, fn = ctypes.c_int(-1), ctypes.c_int(-1)
    assert _hip.lib().frtm_target_apply_grouped_tiles(G, c, h, w, ctypes.byref(fm), ctypes.byref(fn)) == 0
    return fm.value, fn.value


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the table reaches every form
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_query_is_declared_bound_and_the_literal_rule():
    import os
    import re
    from frtm_vos_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = 'frtm_target_apply_grouped_tiles'
    assert re.search(r'\bint %s\s*\(' % name, open(os.path.join(root, 'include', 'frtm_hip.h')).read()) and name in _hip.SIGNATURES
    src = open(os.path.join(root, 'frtm-vos_amd', 'csrc', 'target_apply_grouped.hip')).read()
    launcher = src[src.index('int frtm_target_apply_grouped('):]
    assert name + '(G, c, h, w, &FM, &FN)' in launcher and 'ceil_div(c, 32)' not in launcher and '>= 256' not in launcher   # one definition
    for G in (1, 2, 3, 4, 5, 9, 10, 127, 128, 129, 255, 256, 257, 65535):
        for c in (1, 31, 32, 33, 64, 65, 96, 97, 128):
            for h, w in ((1, 1), (8, 8), (13, 5), (8, 16), (3, 43), (30, 54), (4096, 4096)):
                hw = h * w
                assert _tiles(G, c, h, w) == (-(-c // 32), 2 if -(-hw // 64) * G >= 256 else 1), (G, c, h, w)
    L = _hip.lib()
    fm, fn = ctypes.c_int(), ctypes.c_int()
    for G, c, h, w in ((0, 8, 4, 4), (65536, 8, 4, 4), (1, 0, 4, 4), (1, 129, 4, 4), (1, 8, 0, 4), (1, 8, 4097, 4096)):
        assert L.frtm_target_apply_grouped_tiles(G, c, h, w, ctypes.byref(fm), ctypes.byref(fn)) == -1, (G, c, h, w)
    assert L.frtm_target_apply_grouped_tiles(1, 8, 4, 4, None, ctypes.byref(fn)) == -1


def test_the_table_reaches_every_form_and_edge():
    forms, fn1_c = {}, set()
    for name, (Cin, c, h, w, frames, fop, extra, offset) in R.CASES.items():
        fm, fn = _tiles(len(fop), c, h, w)
        forms.setdefault((fm, fn), []).append(name)
        if fn == 1:
            fn1_c.add(c)
        assert Cin % 32 == 0 and max(fop) < frames and sorted(set(fop)) == list(range(frames)), name       # every frame is read
        assert 4 * max(len(fop) * c * h * w, frames * (Cin * h * w + extra)) <= 4 << 20, name               # the largest tensor: a few MB
    print({k: v for k, v in sorted(forms.items())})
    assert sorted(forms) == [(fm, fn) for fm in (1, 2, 3, 4) for fn in (1, 2)]
    assert fn1_c >= {1, 8, 31, 32, 33, 63, 65, 96, 97, 127, 128} and fn1_c >= {1, 15, 16, 17, 128}
    for fm in (1, 2, 3, 4):
        for table, fn in ((R.FN1_PER_FM, 1), (R.FN2_PER_FM, 2)):
            Cin, c, h, w, frames, fop, _, _ = R.CASES[table[fm]]
            assert _tiles(len(fop), c, h, w) == (fm, fn) and len(fop) >= 3
    name, below, above = R.SWITCH
    Cin, c, h, w, frames, fop, _, _ = R.CASES[name]
    assert h * w == 64 and (below, above) == (255, 256) == (len(fop) - 1, len(fop))
    assert _tiles(below, c, h, w)[1] == 1 and _tiles(above, c, h, w)[1] == 2
    rows = list(R.CASES.values())
    assert {r[0] for r in rows} == {32, 64, 96, 160}                                                         # 1, 2, 3, 5 chunks
    assert {r[2] * r[3] for r in rows} >= {1, 15, 16, 17, 31, 32, 33, 63, 64, 65}
    assert any(r[2] == 1 and r[3] > 1 for r in rows) and any(r[3] == 1 and r[2] > 1 for r in rows)
    assert any(r[3] == 5 and r[2] >= 4 for r in rows) and any(r[3] == 7 and r[2] >= 3 for r in rows)          # a 16-pixel tile on 4 and on 3 rows
    assert any((r[0] * r[2] * r[3] + r[6]) % 4 != 0 and r[4] > 1 for r in rows)                               # a pitch that is no multiple of 4 floats
    assert any(r[7] for r in rows) and all(len(r[5]) >= 2 for r in rows if r[7])
    Cin, c, h, w, frames, fop, _, _ = R.CASES[R.SKIP]
    assert len(fop) == 5 and frames == 3


def test_neighbouring_pairs_share_neither_frame_nor_weights_in_the_large_launches():
    for name in R.FN2_PER_FM.values():
        case = R.make(name)
        G = len(case.fop)
        assert case.sets == R.WEIGHT_SETS and len(R.combos(case)) == 15
        for p in range(G - 1):
            assert case.fop[p] != case.fop[p + 1] and case.wop[p] != case.wop[p + 1], (name, p)
    for name in R.CASES:
        case = R.make(name)
        for p in range(len(case.fop) - 1):
            assert (case.fop[p], case.wop[p]) != (case.fop[p + 1], case.wop[p + 1]), (name, p)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the data tells a mix-up apart
# ---------------------------------------------------------------------------------------------------------------------------------
def _misses(right, wrong, c):
    """Does `wrong` = (cft64, s64) miss `right` = reference(...) by more than MIXUP_FACTOR bounds somewhere, in cft and in the scores?
    The scores' bound is taken at the right features (what a right kernel would have read)."""
    cft64, b1, s64, carried = right[:4]
    b2 = R.gamma(9 * c + 1) * F.conv2d(cft64.abs(), right[4].double().abs(), padding=1) + carried
    r1 = float(((wrong[0] - cft64).abs() / b1.clamp(min=1e-300)).max())
    r2 = float(((wrong[1] - s64).abs() / b2.clamp(min=1e-300)).max())
    return min(r1, r2)


@pytest.mark.parametrize('name', list(R.CASES))
def test_a_mixed_up_pair_frame_or_layout_misses_the_bound_a_hundredfold(name):
    case, other = R.make(name), R.make(name, draw=1)
    Cin, c = case.Cin, case.c
    worst = {}
    for (f, s), pairs in R.combos(case).items():
        X, w1T, w2 = case.X[f], case.w1T[s], case.w2[s]
        right = R.reference(Cin, c, X, w1T, w2) + (w2,)
        assert bool((right[1] > 0).all()) and bool((right[3] > 0).all())                  # (no bound is 0: no element is exempt)
        s_n, f_n = (s + 1) % case.sets, (f + 1) % case.frames
        wrong = {'weights': R.reference(Cin, c, X, *((case.w1T[s_n], case.w2[s_n]) if case.sets > 1 else (other.w1T[0], other.w2[0]))),
                 'frame': R.reference(Cin, c, case.X[f_n] if case.frames > 1 else other.X[0], w1T, w2)}
        # one wrong table at a time: the projection of the neighbour under this pair's filter, and the reverse
        wrong['w1T only'] = R.reference(Cin, c, X, case.w1T[s_n] if case.sets > 1 else other.w1T[0], w2)
        if c > 1:
            wrong['layout'] = R.reference(Cin, c, X, w1T.reshape(c, Cin).t(), w2)
        for kind, got in wrong.items():
            worst[kind] = min(worst.get(kind, float('inf')), _misses(right, (got[0], got[2]), c))
        w2_n = case.w2[s_n] if case.sets > 1 else other.w2[0]                             # (the features right, the filter the neighbour's)
        s_wrong = F.conv2d(right[0], w2_n.double(), padding=1)
        b2 = R.gamma(9 * c + 1) * F.conv2d(right[0].abs(), w2.double().abs(), padding=1) + right[3]
        worst['w2 only'] = min(worst.get('w2 only', float('inf')), float(((s_wrong - right[2]).abs() / b2).max()))
    print(name, {k: '%.1e' % v for k, v in worst.items()})
    assert all(v > R.MIXUP_FACTOR for v in worst.values()), worst


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the definition is the per-pair path
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['c33-9x7', 'c96-3x5'])
def test_the_reference_is_the_per_pair_apply_in_float64(name):
    case = R.make(name)
    for p, (f, s) in enumerate(zip(case.fop, case.wop)):
        ft = case.X[f:f + 1].double()
        project = case.w1T[s].double().t().reshape(case.c, case.Cin, 1, 1)                # nn.Conv2d(Cin, c, 1, bias=False).weight
        cft = F.conv2d(ft, project)
        scores = F.conv2d(cft, case.w2[s].double(), padding=1)                            # nn.Conv2d(c, 1, 3, padding=1, bias=False)
        cft64, b1, s64, carried = R.reference(case.Cin, case.c, case.X[f], case.w1T[s], case.w2[s])
        assert float((cft64 - cft).abs().max()) <= 1e-12 and float((s64 - scores).abs().max()) <= 1e-12
        # _bounds returns the same two results, and its bounds are the docstring's
        got = R._bounds(case.Cin, case.c, case.X[f], case.w1T[s], case.w2[s], cft.float())
        assert torch.equal(got[0], cft64) and torch.equal(got[2], s64) and torch.equal(got[1], b1)
        want = R.gamma(9 * case.c + 1) * F.conv2d(cft.float().double().abs(), case.w2[s].double().abs(), padding=1) + carried
        assert torch.equal(got[3], want) and tuple(got[3].shape) == (1, 1, case.h, case.w)
    two = R._bounds(case.Cin, case.c, case.X[f], case.w1T[s], case.w2[s], torch.cat([cft.float(), 2 * cft.float()]))[3]
    assert tuple(two.shape) == (2, 1, case.h, case.w) and float((two[:1] / want - 1).abs().max()) < 1e-12 and bool((two[1] > two[0]).all())


def test_gamma():
    assert R.gamma(1) == R.U / (1 - R.U) and abs(R.gamma(1025) / (1025 * 2.0 ** -24) - 1) < 1e-4
