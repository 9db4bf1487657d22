"""Both kernels of grouped target-model scoring (csrc/target_apply_grouped.hip) against their float64 definition at every compiled tile form
and at the edges of both: k_grouped_project<FM, FN> in its eight forms with the zeroed rows c .. BM - 1, the staging and store guards, one, two
and odd chunk counts; k_grouped_scores with empty and ragged channel groups, maps one pixel high or wide and below a tile.  The case table,
the definition and the bounds are tests/_grouped_refs.py, pinned on the CPU by tests/test_grouped_refs.py (which also asserts that the table
reaches every form and that its data tells a mixed-up pair, frame or weight layout from the right result by 100 bounds or more).

Gate: error / bound <= 1 with the two derived bounds of tests/_grouped_refs.py (Higham's gamma(Cin + 1) for the projection, gamma(9c + 1) plus
the carried term for the scores).  Nothing here is measured into a tolerance.

Output hygiene: cft and scores are handed in as workspaces, each between two NaN guard bands of 64 floats which must stay NaN; for the
accuracy tests they are NaN-filled and every element must end up written.  The skip rule (a pair whose table entry names none of the F frames
leaves its slices of cft AND of scores untouched) is tested with finite sentinels, one bit pattern per buffer: under a NaN pre-fill, scores
computed from unwritten features would be NaN as well and pass for untouched.

Pairs do not interact: a pair's result is bitwise the same alone (G = 1, always the 32-pixel tile), inside its launch (for the 'fn2' cases the
64-pixel tile) and with the tables reversed; the first 255 pairs of the 256-pair launch equal the 255-pair launch across the FN switch.

No test asserts a time; the module (32 tests) ran in 3.1 to 3.5 s on an MI355X.  Worst error / bound per form <FM,FN> over the cases of the
table that run it, projection and scores, as test_against_fp64 prints them (`pytest -s`); the same figures in two runs:
    <1,1> 0.072, 4.98e-03   <2,1> 0.093, 1.07e-03   <3,1> 0.055, 6.81e-04   <4,1> 0.095, 3.99e-04
    <1,2> 0.104, 8.33e-03   <2,2> 0.057, 1.34e-03   <3,2> 0.123, 5.58e-04   <4,2> 0.057, 5.40e-04
    through discriminator.apply_grouped (Cin 64, c 8, 6 x 7): 0.034, 3.26e-03
The scores sit far inside their bound because it is a worst case over 9c products of mixed sign plus the projection's whole bound carried
through |w2|; a dropped channel or tap still misses it by a factor of 10 to 100 at these shapes (a term is some 1e-2, the bound 1e-4 to 1e-3).
With the skip missing from k_grouped_scores (the code before this module), test_a_pair_whose_entry_names_no_frame_is_skipped fails at all
three entries on the scores of pair 1 -- scored from the sentinel features -- and every other test of the module passes.
"""
import pytest
import torch

import _grouped_refs as R
from test_solver_kernels_gpu import _bits, _Buf

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CFT_SENTINEL, SCORES_SENTINEL = 0x42F6E979, 0xC1E6B852          # 123.456 and -28.84: finite, neither 0 nor NaN, distinct per buffer
INT_MAX = 2 ** 31 - 1


def _offset(t, by):
    """t on the device, starting `by` floats into its own storage: by = 1 gives an address that is 4-byte but not 16-byte aligned."""
    store = torch.empty(t.numel() + by, device=DEV)
    out = store[by:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 4 * by
    return out


class _Device:
    """A case's inputs on the device, uploaded once: feats (frames, Cin, h, w) with the case's pitch, the weight sets, and -- where the case
    asks for it -- feats, w1T[1 % sets] and w2[2 % sets] one float into their storage."""

    def __init__(self, case):
        self.case = case
        by = 1 if case.offset else 0
        store = _offset(case.store.reshape(-1), by)
        self.feats = store.as_strided((case.frames, case.Cin, case.h, case.w), (case.pitch, case.h * case.w, case.w, 1), store.storage_offset())
        assert self.feats.data_ptr() % 16 == 4 * by and torch.equal(self.feats.cpu(), case.X)
        self.w1T = [_offset(t, by if k == 1 % case.sets else 0) for k, t in enumerate(case.w1T)]
        self.w2 = [_offset(t, by if k == 2 % case.sets else 0) for k, t in enumerate(case.w2)]

    def run(self, pairs, table=None, fill=None):
        """The kernels on the pairs `pairs` (indices into the case's tables, in this order) into guarded workspaces -> (cft, scores) _Bufs.
        table: the frame table handed to the launch instead of the pairs' own entries; fill: (cft, scores) int32 bit patterns, else NaN."""
        from frtm_vos_amd import ops
        case, G = self.case, len(pairs)
        cft, s = _Buf(G, case.c, case.h, case.w), _Buf(G, 1, case.h, case.w)
        if fill is not None:
            for buf, bits in zip((cft, s), fill):
                _bits(buf.t).fill_(bits - (1 << 32) if bits >= 1 << 31 else bits)
                buf.before = buf.t.clone()
        fop = torch.tensor([case.fop[p] for p in pairs] if table is None else table, dtype=torch.int32, device=DEV)
        w1T, w2 = [self.w1T[case.wop[p]] for p in pairs], [self.w2[case.wop[p]] for p in pairs]
        got = ops.target_apply_grouped(self.feats, fop, ops.pointer_table(w1T, DEV), ops.pointer_table(w2, DEV), case.c, cft=cft.t, scores=s.t)
        torch.cuda.synchronize()
        assert got[0].data_ptr() == cft.t.data_ptr() and got[1].data_ptr() == s.t.data_ptr()
        return cft, s


_devices = {}


def _dev(name):
    if name not in _devices:
        _devices[name] = _Device(R.make(name))
    return _devices[name]


def _form(case, G):
    import ctypes
    from frtm_vos_amd import _hip
    fm, fn = ctypes.c_int(), ctypes.c_int()
    assert _hip.lib().frtm_target_apply_grouped_tiles(G, case.c, case.h, case.w, ctypes.byref(fm), ctypes.byref(fn)) == 0
    return fm.value, fn.value


def _ratios(case, pairs, cft, s):
    """Worst error / bound of the launch's pairs: (projection, scores).  One float64 reference per distinct (frame, weight set)."""
    worst = [0.0, 0.0]
    where = {}
    for k, p in enumerate(pairs):
        where.setdefault((case.fop[p], case.wop[p]), []).append(k)
    for (f, ws), rows in where.items():
        got_cft, got_s = cft[rows], s[rows]
        cft64, b1, s64, b2 = R._bounds(case.Cin, case.c, case.X[f], case.w1T[ws], case.w2[ws], got_cft)
        n = len(rows)
        worst[0] = max(worst[0], R._worst(got_cft, cft64.expand(n, -1, -1, -1), b1.expand(n, -1, -1, -1)))
        worst[1] = max(worst[1], R._worst(got_s, s64.expand(n, -1, -1, -1), b2))
    return worst


_worst_per_form = {}


@pytest.mark.parametrize('name', list(R.CASES))
def test_against_fp64(name):
    dev = _dev(name)
    case, pairs = dev.case, list(range(len(dev.case.fop)))
    cft, s = dev.run(pairs)
    r1, r2 = _ratios(case, pairs, cft.done().cpu(), s.done().cpu())
    form = _form(case, len(pairs))
    seen = _worst_per_form.setdefault(form, [0.0, 0.0])
    seen[0], seen[1] = max(seen[0], r1), max(seen[1], r2)
    print('FORM <%d,%d> %s: worst error / bound: projection %.3f, scores %.2e' % (form + (name, r1, r2)))
    if name == list(R.CASES)[-1]:
        for k, v in sorted(_worst_per_form.items()):
            print('FORM <%d,%d> over its cases: projection %.3f, scores %.2e' % (k + tuple(v)))
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)


@pytest.mark.parametrize('name', list(R.FN1_PER_FM.values()) + list(R.FN2_PER_FM.values()))
def test_a_pairs_result_does_not_depend_on_the_launch(name):
    """Alone (G = 1), inside the full launch and with the tables reversed: bitwise the same projected features and scores.  Alone: every pair of
    a small launch; of the large ones the first 15 -- every (frame, weight set) they hold -- and the last."""
    dev = _dev(name)
    G = len(dev.case.fop)
    cft, s = (b.done().cpu() for b in dev.run(list(range(G))))
    cft_r, s_r = (b.done().cpu() for b in dev.run(list(range(G - 1, -1, -1))))
    assert torch.equal(_bits(cft_r.flip(0)), _bits(cft)) and torch.equal(_bits(s_r.flip(0)), _bits(s))
    for p in sorted(set(range(min(G, 15))) | {G - 1}):
        cft_1, s_1 = (b.done().cpu() for b in dev.run([p]))
        assert torch.equal(_bits(cft_1[0]), _bits(cft[p])) and torch.equal(_bits(s_1[0]), _bits(s[p])), p
    assert not torch.equal(cft[0], cft[1]) and not torch.equal(s[0], s[1])


def test_the_first_255_pairs_are_bitwise_the_same_on_either_side_of_the_tile_switch():
    name, below, above = R.SWITCH
    dev = _dev(name)
    assert _form(dev.case, below)[1] == 1 and _form(dev.case, above)[1] == 2
    cft_a, s_a = (b.done().cpu() for b in dev.run(list(range(above))))
    cft_b, s_b = (b.done().cpu() for b in dev.run(list(range(below))))
    assert torch.equal(_bits(cft_a[:below]), _bits(cft_b)) and torch.equal(_bits(s_a[:below]), _bits(s_b))


@pytest.mark.parametrize('entry', ['F', -1, INT_MAX])
def test_a_pair_whose_entry_names_no_frame_is_skipped(entry):
    """5 pairs on 3 frames; the entries of pairs 1 and 3 name no frame.  Both workspaces hold finite sentinels: the skipped pairs' slices of cft
    and of scores and the guards are bit for bit what they were, every other pair is bitwise what the launch with the valid table gives."""
    dev = _dev(R.SKIP)
    case = dev.case
    pairs, skipped = list(range(5)), (1, 3)
    cft_v, s_v = dev.run(pairs, fill=(CFT_SENTINEL, SCORES_SENTINEL))
    cft_v.guards(), s_v.guards()
    for buf in (cft_v, s_v):                                     # the valid launch overwrites every sentinel
        assert not bool((_bits(buf.t) == _bits(buf.before)).any())
    table = list(case.fop)
    for p in skipped:
        table[p] = case.frames if entry == 'F' else entry
    cft, s = dev.run(pairs, table=table, fill=(CFT_SENTINEL, SCORES_SENTINEL))
    cft.guards(), s.guards()
    assert int(_bits(cft.before)[0, 0, 0, 0]) == CFT_SENTINEL and int(_bits(s.before)[0, 0, 0, 0]) == SCORES_SENTINEL - (1 << 32)
    for p in pairs:
        if p in skipped:
            assert torch.equal(_bits(cft.t[p]), _bits(cft.before[p])), 'projected features of skipped pair %d written' % p
            assert torch.equal(_bits(s.t[p]), _bits(s.before[p])), 'scores of skipped pair %d written' % p
        else:
            assert torch.equal(_bits(cft.t[p]), _bits(cft_v.t[p])) and torch.equal(_bits(s.t[p]), _bits(s_v.t[p])), p


def test_two_launches_are_bitwise_equal():
    dev = _dev(R.FN2_PER_FM[2])
    pairs = list(range(len(dev.case.fop)))
    a, b = dev.run(pairs), dev.run(pairs)
    assert a[0].t.data_ptr() != b[0].t.data_ptr()
    assert torch.equal(_bits(a[0].done()), _bits(b[0].done())) and torch.equal(_bits(a[1].done()), _bits(b[1].done()))


def test_apply_grouped_follows_a_replaced_filter_and_leaves_the_other_models_alone():
    """discriminator.apply_grouped with a kept cache: a filter weight replaced by a NEW tensor moves its address, so the pointer tables must be
    rebuilt -- the next call scores that model with the new filter, within the bound, and the other two bitwise as before."""
    from frtm_vos_amd.model.discriminator import Discriminator, apply_grouped
    Cin, c, h, w = 64, 8, 6, 7
    g = torch.Generator().manual_seed(11)
    discs = []
    for _ in range(3):
        d = Discriminator(in_channels=Cin, c_channels=c, init_iters=(2, 3), update_iters=(3,), memory_size=4, train_skipping=1,
                          pixel_weighting=dict(method='hinge', tf=0.1), device=DEV, layer='layer4')
        d.project.weight.data.copy_(torch.randn(c, Cin, 1, 1, generator=g) / Cin ** 0.5)
        d.filter.weight.data.copy_(torch.randn(1, c, 3, 3, generator=g) / (9 * c) ** 0.5)
        d._invalidate()
        discs.append(d)
    X = torch.randn(3, Cin, h, w, generator=g).relu()
    feats, cache = X.to(DEV), {}

    def check(scores, cft):
        for i, d in enumerate(discs):
            w1T = d.project.weight.data.view(c, Cin).t().cpu()
            cft64, b1, s64, b2 = R._bounds(Cin, c, X[i], w1T, d.filter.weight.data.cpu(), cft[i])
            r1, r2 = R._worst(cft[i], cft64, b1), R._worst(scores[i], s64, b2)
            print('model %d: worst error / bound: projection %.3f, scores %.2e' % (i, r1, r2))
            assert r1 <= 1.0 and r2 <= 1.0, (i, r1, r2)

    cft0, s0 = (t.cpu() for t in apply_grouped(discs, feats, 1, cache))
    check(s0, cft0)
    tables = (cache['w1T'], cache['w2'])
    cft1, s1 = (t.cpu() for t in apply_grouped(discs, feats, 1, cache))                       # nothing moved: the tables are kept
    assert cache['w1T'] is tables[0] and cache['w2'] is tables[1] and torch.equal(_bits(s1), _bits(s0))
    old = discs[1].filter.weight.data
    discs[1].filter.weight.data = (torch.randn(1, c, 3, 3, generator=g) / (9 * c) ** 0.5).to(DEV)
    assert discs[1].filter.weight.data_ptr() != old.data_ptr()
    cft2, s2 = (t.cpu() for t in apply_grouped(discs, feats, 1, cache))
    check(s2, cft2)                                                                           # (model 1 against its NEW filter)
    assert cache['w2'] is not tables[1]
    assert torch.equal(_bits(cft2), _bits(cft0)) and not torch.equal(s2[1], s0[1])
    for i in (0, 2):
        assert torch.equal(_bits(s2[i]), _bits(s0[i])), i
    assert all(d.frame_num == 3 for d in discs)
    torch.cuda.synchronize()
    del old
