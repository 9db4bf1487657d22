"""Ragged StreamPool groups on the GPU: the four kernels of csrc/ragged_group.hip, the refiner with a sample-to-frame table and the pool
with ``ragged_groups``.

Kernel level.  Each indexed refiner kernel against its float64 definition (tests/_refiner_refs.py on the frame-expanded inputs) under the
gate of tests/test_refiner_kernels_gpu.py, max|hip - ref64| <= max(4 * max|torch32 - ref64|, 1e-6 * max|ref64|), cab_combine with that
module's 2^-21 * max|shallow| floor for its __expf; every output NaN-prefilled between 64-float guard bands.  Bitwise: with the table
s // group each kernel equals the existing entry point; the ragged merge on equal counts equals frtm_track_merge, and on unequal counts
every frame equals a one-frame frtm_track_merge; a sample's output does not depend on the other frames of the launch.  A table entry
outside [0, F) is the specified skip path: that sample stays NaN, the others are written, the guards stay intact.

Refiner and pool level: the bounds of tests/test_hip_parity.py::test_segnetwork_frame_window_equals_per_frame_calls and the bars of
tests/test_stream_pool_gpu.py::_compare.  No test asserts a time."""
from collections import OrderedDict

import pytest
import torch

import _refiner_refs as R
from test_refiner_kernels_gpu import EXPF_TERM, _Out, _call, _check, _gen, _legs, _randn, _uniform
from test_stream_pool_gpu import SIZE, _compare, _literal_loop, _params

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = 'cuda:0'


def _table(counts):
    from frtm_vos_amd import ops
    return ops.RaggedTable(counts, DEV)


def _idx(counts):
    return torch.tensor([f for f, c in enumerate(counts) for _ in range(c)])


def _i32(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


# ---------------------------------------------------------------------------------------------------------------------------------
# the indexed refiner kernels: inputs on the host, one launch through the C entry point into a guarded output
# ---------------------------------------------------------------------------------------------------------------------------------
def _tse_inputs(C, Hh, Ww, half, counts):
    g = _gen(C, Hh, Ww, half, *counts)
    h, w = ((Hh + 1) // 2, (Ww + 1) // 2) if half else (Hh, Ww)
    return _randn(g, len(counts), C, Hh, Ww), _randn(g, C) * 0.5, _randn(g, C, 9) * 0.3, _randn(g, sum(counts), h, w)


def _tse_launch(base, bias, ws, scores, frame_of, out):
    n, (h, w), (F_, C, Hh, Ww) = scores.shape[0], scores.shape[-2:], base.shape
    _call('frtm_tse_inject_indexed', base.to(DEV), bias.to(DEV), ws.to(DEV), scores.to(DEV), n, frame_of, F_, C, h, w, Hh, Ww, out.t)


def _gate_inputs(oc, counts):
    g = _gen(oc, *counts)
    return (_randn(g, sum(counts), oc), _randn(g, len(counts), oc), _randn(g, 2 * oc, oc) / (2 * oc) ** 0.5, _randn(g, oc) * 0.3,
            _randn(g, oc, oc) / oc ** 0.5, _randn(g, oc) * 0.3)


def _gate_launch(sp, dp, W1, b1, W2, b2, row_of, out):
    _call('frtm_cab_gate_indexed', sp.to(DEV), dp.to(DEV), row_of, dp.shape[0], W1.to(DEV), b1.to(DEV), W2.to(DEV), b2.to(DEV), sp.shape[0],
          sp.shape[1], out.t)


def _combine_inputs(C, hd, wd, Hh, Ww, counts):
    g = _gen(C, hd, wd, Hh, Ww, *counts)
    n = sum(counts)
    return _randn(g, n, C, Hh, Ww), _uniform(g, -4, 4, n, C), _randn(g, len(counts), C, hd, wd)


def _combine_launch(shallow, gate, deeper, entry_of, out):
    n, C, Hh, Ww = shallow.shape
    _call('frtm_cab_combine_indexed', shallow.to(DEV), gate.to(DEV), deeper.to(DEV), entry_of, deeper.shape[0], n, C, deeper.shape[2],
          deeper.shape[3], Hh, Ww, out.t)


TSE_CASES = [(5, 9, 33, True, (3, 1, 2)), (4, 1, 1, False, (1, 2)), (3, 61, 107, False, (2, 1, 1)), (64, 30, 54, True, (1, 3))]


@pytest.mark.parametrize('C,Hh,Ww,half,counts', TSE_CASES)
def test_tse_inject_indexed_against_fp64(C, Hh, Ww, half, counts):
    base, bias, ws, scores = _tse_inputs(C, Hh, Ww, half, counts)
    out = _Out(sum(counts), C, Hh, Ww)
    _tse_launch(base, bias, ws, scores, _table(counts).frame_of, out)
    idx = _idx(counts)
    r64, r32 = _legs(lambda b, *a: R.tse_inject(b[idx.to(b.device)], *a, 1), base, bias, ws, scores)
    _check('k_tse_inject_indexed', 'C%d %dx%d half %d counts %r' % (C, Hh, Ww, half, counts), out.done(), r64, r32)


@pytest.mark.parametrize('oc', [4, 60, 64, 68, 256])
def test_cab_gate_indexed_against_fp64(oc):
    counts = (3, 1, 2)
    args = _gate_inputs(oc, counts)
    out = _Out(sum(counts), oc)
    _gate_launch(*args, _table(counts).frame_of, out)
    idx = _idx(counts)
    r64, r32 = _legs(lambda s, d, *a: R.cab_gate(s, d[idx.to(d.device)], 0, *a), *args)
    _check('k_cab_gate_indexed', 'oc%d counts %r' % (oc, counts), out.done(), r64, r32)


# (C, hd, wd, H, W, counts): the pooled vector of the product, then a deeper MAP per frame
COMBINE_CASES = [(5, 1, 1, 16, 64, (3, 1, 2)), (5, 1, 1, 17, 130, (3, 1, 2)), (5, 1, 1, 33, 1, (3, 1, 2)), (4, 8, 32, 16, 64, (1, 2))]


@pytest.mark.parametrize('C,hd,wd,Hh,Ww,counts', COMBINE_CASES)
def test_cab_combine_indexed_against_fp64(C, hd, wd, Hh, Ww, counts):
    shallow, gate, deeper = _combine_inputs(C, hd, wd, Hh, Ww, counts)
    out = _Out(sum(counts), C, Hh, Ww)
    _combine_launch(shallow, gate, deeper, _table(counts).frame_of, out)
    idx = _idx(counts)
    r64, r32 = _legs(lambda s, g, d: R.cab_combine(s, g, d[idx.to(d.device)], 0), shallow, gate, deeper)
    _check('k_cab_combine_indexed', 'C%d (%d,%d)->(%d,%d) counts %r' % (C, hd, wd, Hh, Ww, counts), out.done(), r64, r32,
           floor=EXPF_TERM * float(shallow.abs().max()))


@pytest.mark.parametrize('group', [1, 2, 3])
def test_indexed_kernels_equal_the_uniform_ones_bit_for_bit(group):
    """The table s // group: the outputs of the existing entry points, bit for bit."""
    counts = (group, group)
    n, frame_of = 2 * group, _table(counts).frame_of
    assert frame_of.tolist() == [s // group for s in range(n)]
    base, bias, ws, scores = _tse_inputs(5, 9, 33, True, counts)
    out, ref = _Out(n, 5, 9, 33), _Out(n, 5, 9, 33)
    _tse_launch(base, bias, ws, scores, frame_of, out)
    _call('frtm_tse_inject', base.to(DEV), bias.to(DEV), ws.to(DEV), scores.to(DEV), n, group, 5, 5, 17, 9, 33, ref.t)
    assert torch.equal(out.done(), ref.done())
    sp, dp, W1, b1, W2, b2 = _gate_inputs(68, counts)
    out, ref = _Out(n, 68), _Out(n, 68)
    _gate_launch(sp, dp, W1, b1, W2, b2, frame_of, out)
    _call('frtm_cab_gate', sp.to(DEV), dp.to(DEV), group, W1.to(DEV), b1.to(DEV), W2.to(DEV), b2.to(DEV), n, 68, ref.t)
    assert torch.equal(out.done(), ref.done())
    for hd, wd in ((1, 1), (8, 32)):
        shallow, gate, deeper = _combine_inputs(5, hd, wd, 17, 64, counts)
        out, ref = _Out(n, 5, 17, 64), _Out(n, 5, 17, 64)
        _combine_launch(shallow, gate, deeper, frame_of, out)
        _call('frtm_cab_combine', shallow.to(DEV), gate.to(DEV), deeper.to(DEV), n, 5, hd, wd, group, 17, 64, ref.t)
        assert torch.equal(out.done(), ref.done())


def test_a_samples_output_does_not_depend_on_the_other_frames():
    """Counts (3, 1, 2): every frame's samples are bit for bit those of a launch that holds this frame alone."""
    counts = (3, 1, 2)
    frame_of = _table(counts).frame_of
    starts = [0, 3, 4, 6]
    base, bias, ws, scores = _tse_inputs(5, 9, 33, True, counts)
    sp, dp, W1, b1, W2, b2 = _gate_inputs(68, counts)
    shallow, gate, deeper = _combine_inputs(5, 1, 1, 17, 130, counts)
    o_t, o_g, o_c = _Out(6, 5, 9, 33), _Out(6, 68), _Out(6, 5, 17, 130)
    _tse_launch(base, bias, ws, scores, frame_of, o_t)
    _gate_launch(sp, dp, W1, b1, W2, b2, frame_of, o_g)
    _combine_launch(shallow, gate, deeper, frame_of, o_c)
    t_all, g_all, c_all = o_t.done(), o_g.done(), o_c.done()
    for f, n_f in enumerate(counts):
        a, b = starts[f], starts[f + 1]
        own = _table((n_f,)).frame_of
        o_t, o_g, o_c = _Out(n_f, 5, 9, 33), _Out(n_f, 68), _Out(n_f, 5, 17, 130)
        _tse_launch(base[f:f + 1], bias, ws, scores[a:b], own, o_t)
        _gate_launch(sp[a:b], dp[f:f + 1], W1, b1, W2, b2, own, o_g)
        _combine_launch(shallow[a:b], gate[a:b], deeper[f:f + 1], own, o_c)
        assert torch.equal(o_t.done(), t_all[a:b]) and torch.equal(o_g.done(), g_all[a:b]) and torch.equal(o_c.done(), c_all[a:b]), f
    assert not torch.equal(t_all[0], t_all[3])


def _skipped(out, sample):
    """The guards are intact, sample ``sample`` is still all NaN and every other element was written; returns the output."""
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.buf[:out.lo]).all()) and bool(torch.isnan(out.buf[out.lo + out.t.numel():]).all()), 'write outside the output'
    assert bool(torch.isnan(out.t[sample]).all()), 'the sample without a frame was written'
    keep = [s for s in range(out.t.shape[0]) if s != sample]
    assert not bool(torch.isnan(out.t[keep]).any()), 'output element not written'
    return out.t, keep


def test_a_sample_whose_entry_names_no_frame_is_skipped():
    """The specified skip path (frtm_target_apply_grouped's rule for pairs): entry 3 of the table is F = 3 -- one past the last frame."""
    counts, bad = (3, 1, 2), 3
    entries = _idx(counts).tolist()
    entries[bad] = len(counts)
    frame_of, idx = _i32(entries), _idx(counts)
    base, bias, ws, scores = _tse_inputs(5, 9, 33, True, counts)
    out = _Out(6, 5, 9, 33)
    _tse_launch(base, bias, ws, scores, frame_of, out)
    got, keep = _skipped(out, bad)
    r64, r32 = _legs(lambda b, *a: R.tse_inject(b[idx.to(b.device)], *a, 1), base, bias, ws, scores)
    _check('k_tse_inject_indexed', 'entry %d = F' % bad, got[keep], r64[keep], r32[keep])
    args = _gate_inputs(68, counts)
    out = _Out(6, 68)
    _gate_launch(*args, frame_of, out)
    got, keep = _skipped(out, bad)
    r64, r32 = _legs(lambda s, d, *a: R.cab_gate(s, d[idx.to(d.device)], 0, *a), *args)
    _check('k_cab_gate_indexed', 'entry %d = F' % bad, got[keep], r64[keep], r32[keep])
    shallow, gate, deeper = _combine_inputs(5, 1, 1, 17, 130, counts)
    out = _Out(6, 5, 17, 130)
    _combine_launch(shallow, gate, deeper, frame_of, out)
    got, keep = _skipped(out, bad)
    r64, r32 = _legs(lambda s, g, d: R.cab_combine(s, g, d[idx.to(d.device)], 0), shallow, gate, deeper)
    _check('k_cab_combine_indexed', 'entry %d = F' % bad, got[keep], r64[keep], r32[keep], floor=EXPF_TERM * float(shallow.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the ragged merge
# ---------------------------------------------------------------------------------------------------------------------------------
def _uniform_merge(logits, frames, n, HW):
    masks, counts = _Out(frames * (n + 1), HW), torch.full((frames * (n + 1),), -7, dtype=torch.int32, device=DEV)
    _call('frtm_track_merge', logits, frames, n, HW, masks.t, None, None, 0, counts, 0.5)
    return masks.done(), counts


@pytest.mark.parametrize('HW', [1, 255, 257, 25680])
def test_ragged_merge_on_equal_counts_is_track_merge(HW):
    frames, n = 2, 3
    logits = (_randn(_gen(HW, 7), frames * n, HW) * 3).to(DEV)
    ref_m, ref_c = _uniform_merge(logits, frames, n, HW)
    masks, counts = _Out(frames * (n + 1), HW), torch.full((frames * (n + 1),), -7, dtype=torch.int32, device=DEV)
    _call('frtm_track_merge_ragged', logits, frames, _table((n,) * frames).first, HW, masks.t, counts, 0.5)
    assert torch.equal(masks.done(), ref_m) and torch.equal(counts, ref_c)
    assert int(ref_c.sum()) > 0 or HW == 1


@pytest.mark.parametrize('counts', [(1, 3, 2), (15, 1)])
def test_ragged_merge_equals_the_per_frame_merges(counts):
    from frtm_vos_amd import ops
    Hh, Ww = 33, 47                                                        # 1551 pixels: two workgroups per frame, a tail in the second
    table = _table(counts)
    logits = (_randn(_gen(*counts), table.n, 1, Hh, Ww) * 3).to(DEV)
    masks = _Out(table.n + table.F, Hh, Ww)
    cnt = torch.full((table.n + table.F,), -7, dtype=torch.int32, device=DEV)
    ops.track_merge_ragged(logits, table, masks.t, cnt)
    got = masks.done().clone()
    for f, n_f in enumerate(counts):
        a, b = table.planes(f)
        assert b - a == n_f + 1
        ref_m, ref_c = _uniform_merge(logits[table.starts[f]:table.starts[f + 1]].reshape(n_f, Hh * Ww), 1, n_f, Hh * Ww)
        assert torch.equal(got[a:b].reshape(n_f + 1, -1), ref_m) and torch.equal(cnt[a:b], ref_c), f
        assert int(ref_c.sum()) > 0
    masks.t.fill_(float('nan'))
    ops.track_merge_ragged(logits, table, masks.t)                         # without counts
    assert torch.equal(masks.done(), got)


def test_ragged_merge_refuses_16_objects_and_skips_a_frame_the_table_breaks():
    from frtm_vos_amd import ops
    with pytest.raises(ValueError, match='15'):
        ops.RaggedTable((2, 16), DEV)
    # first = [0, 3, 20, 6]: frame 0 holds 3 objects; frame 1 would hold 17, frame 2 a negative number: both skipped, nothing touched
    HW = 300
    logits = (_randn(_gen(300), 6, HW) * 3).to(DEV)
    masks, counts = _Out(9, HW), torch.full((9,), -7, dtype=torch.int32, device=DEV)
    _call('frtm_track_merge_ragged', logits, 3, _i32([0, 3, 20, 6]), HW, masks.t, counts, 0.5)
    torch.cuda.synchronize()
    assert bool(torch.isnan(masks.buf[:masks.lo]).all()) and bool(torch.isnan(masks.buf[masks.lo + masks.t.numel():]).all())
    assert bool(torch.isnan(masks.t[4:]).all()) and counts[4:].tolist() == [-7] * 5
    ref_m, ref_c = _uniform_merge(logits[:3], 1, 3, HW)
    assert torch.equal(masks.t[:4], ref_m) and torch.equal(counts[:4], ref_c)


# ---------------------------------------------------------------------------------------------------------------------------------
# the refiner with a table
# ---------------------------------------------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def test_segnetwork_with_a_table_equals_per_frame_calls():
    """The network, taps and bounds of test_segnetwork_frame_window_equals_per_frame_calls, with 1, 3 and 2 objects on the three frames."""
    from frtm_vos_amd.model.seg_network import SegNetwork
    chans = OrderedDict(layer5=40, layer4=24, layer3=16, layer2=8)
    torch.manual_seed(5)
    net = SegNetwork(1, 8, chans, True).eval().to(DEV)
    g = torch.Generator().manual_seed(19)
    size, counts = (96, 140), (1, 3, 2)
    table = _table(counts)
    dims = [((size[0] + 2 ** k - 1) // 2 ** k, (size[1] + 2 ** k - 1) // 2 ** k) for k in (5, 4, 3, 2)]
    feats = {L: torch.relu(torch.randn(3, c, *d, generator=g)).to(DEV) for (L, c), d in zip(chans.items(), dims)}
    scores = torch.randn(table.n, 1, *dims[1], generator=g).to(DEV)
    with torch.no_grad():
        win = net(scores, feats, size, frame_of=table)
        ref = net.forward_torch(scores, feats, size, frame_of=table)
        print('ragged window against forward_torch: rel %.2e' % _rel(win, ref))
        assert tuple(win.shape) == (6, 1) + size and _rel(win, ref) < 2e-4
        for f in range(3):
            a, b = table.starts[f], table.starts[f + 1]
            one = net(scores[a:b], {L: t[f:f + 1] for L, t in feats.items()}, size)
            assert _rel(win[a:b], one) < 1e-5, f
        net.parallel_eager = False
        assert torch.equal(net(scores, feats, size, frame_of=table), win)          # one stream or two: the same launches
        net.parallel_eager = True
        net.use_graphs = True
        for _ in range(3):                                                          # (a uniform window is captured on its second use)
            assert torch.equal(net(scores, feats, size, frame_of=table), win)
        assert net._graphs == {} and net._uses == {}                                # a call with a table captures nothing
        with pytest.raises(ValueError, match='table'):
            net(scores[:5], feats, size, frame_of=table)


# ---------------------------------------------------------------------------------------------------------------------------------
# the pool
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sequences():
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    seqs = [SyntheticSequence('a', 12, SIZE, 1, seed=9), SyntheticSequence('b', 11, SIZE, 2, seed=10),      # b: closed one frame early
            SyntheticSequence('c', 12, SIZE, 3, seed=11), SyntheticSequence('d', 12, SIZE, 2, seed=12, late_object_at=5)]
    for s in seqs:
        s.preload(DEV)
    return seqs


def _pool_run(seqs, grouped, ragged):
    """-> (soft masks per stream and frame, per tick (a stream fell back, growth of refiner_passes, object counts of the tracked streams))."""
    pool = _params().get_stream_pool(max_streams=len(seqs), grouped_apply=grouped, ragged_groups=ragged)
    sids = [pool.open() for _ in seqs]
    soft, ticks = [dict() for _ in seqs], []
    for t in range(max(len(s) for s in seqs)):
        frames, late = {}, False
        for k, seq in enumerate(seqs):
            if t >= len(seq):
                continue
            image, labels, new_objects = seq[t]
            if len(new_objects) > 0:
                late = late or t > 0
                torch.manual_seed(0)
                pool.initialize(sids[k], image, labels, new_objects)
            frames[sids[k]] = image
        before = pool.refiner_passes
        out = pool.step(frames)
        ticks.append((late, pool.refiner_passes - before, sorted(m.shape[0] - 1 for m in out.values())))
        for k, seq in enumerate(seqs):
            if sids[k] in out:
                soft[k][t] = out[sids[k]].clone()
            if t + 1 == len(seq):
                pool.close(sids[k])
    torch.cuda.synchronize()
    assert len(pool) == 0
    return soft, ticks


@pytest.fixture(scope='module')
def literal(sequences):
    return [_literal_loop(s) for s in sequences]


@pytest.fixture(scope='module')
def ragged_grouped(sequences):
    return _pool_run(sequences, True, True)


def _same(a, b):
    for x, y in zip(a, b):
        assert sorted(x) == sorted(y) and len(x) >= 8
        for t in x:
            assert torch.equal(x[t], y[t]), t


def test_ragged_pool_with_grouped_apply_matches_the_literal_loop(ragged_grouped, literal):
    _compare(ragged_grouped[0], literal)


def test_ragged_pool_with_per_pair_apply_matches_the_literal_loop(sequences, literal):
    _compare(_pool_run(sequences, False, True)[0], literal)


def test_one_refiner_pass_per_tick_where_the_uniform_pool_makes_three(sequences, ragged_grouped):
    """Streams with 1, 2, 3 and 2 (before frame 5: 1) objects: on every tick without a fallback the ragged pool calls the refiner once,
    the uniform pool once per distinct object count."""
    checked = 0
    for late, passes, counts in ragged_grouped[1]:
        if counts and not late:
            assert passes == 1 and len(set(counts)) == 3, (passes, counts)
            checked += 1
    assert checked >= 9
    _, ticks = _pool_run(sequences, True, False)
    assert [c for _, _, c in ticks] == [c for _, _, c in ragged_grouped[1]]
    for late, passes, counts in ticks:
        if counts and not late:
            assert passes == len(set(counts)) == 3, (passes, counts)


def test_two_ragged_runs_are_bitwise_equal(sequences, ragged_grouped):
    _same(_pool_run(sequences, True, True)[0], ragged_grouped[0])


def test_a_ragged_pool_of_equal_counts_is_bitwise_the_uniform_pool():
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    seqs = [SyntheticSequence('e%d' % k, 10, SIZE, 2, seed=40 + k) for k in range(3)]
    for s in seqs:
        s.preload(DEV)
    on, ticks_on = _pool_run(seqs, True, True)
    off, ticks_off = _pool_run(seqs, True, False)
    _same(on, off)
    assert ticks_on == ticks_off and all(p == 1 for _, p, c in ticks_on if c)


def test_steady_ragged_ticks_allocate_nothing_on_the_device():
    """tests/test_stream_pool_gpu.py::test_steady_ticks_allocate_nothing_on_the_device with 1, 2 and 3 objects in ONE group."""
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    seqs = [SyntheticSequence('m%d' % k, 17, SIZE, k + 1, seed=20 + k) for k in range(3)]
    for s in seqs:
        s.preload(DEV)
    pool = _params().get_stream_pool(max_streams=3, grouped_apply=True, ragged_groups=True)
    sids = [pool.open() for _ in seqs]

    def tick(t):
        frames = {}
        for sid, seq in zip(sids, seqs):
            image, labels, new_objects = seq[t]
            if len(new_objects) > 0:
                pool.initialize(sid, image, labels, new_objects)
            frames[sid] = image
        return pool.step(frames)

    for t in range(13):
        tick(t)
    torch.cuda.synchronize()
    st0, n0, p0 = torch.cuda.memory_stats(), pool.grouped_launches, pool.refiner_passes
    for t in range(13, 17):
        out = tick(t)
        assert sorted(m.shape[0] for m in out.values()) == [2, 3, 4]
    torch.cuda.synchronize()
    st1 = torch.cuda.memory_stats()
    print('cache allocations over 4 ticks: %d, device mallocs: %d' % (st1['allocation.all.allocated'] - st0['allocation.all.allocated'],
                                                                       st1['num_device_alloc'] - st0['num_device_alloc']))
    assert pool.grouped_launches == n0 + 4 and pool.refiner_passes == p0 + 4      # one group per tick: all three streams
    assert st1['num_device_alloc'] == st0['num_device_alloc']
    assert st1['reserved_bytes.all.allocated'] == st0['reserved_bytes.all.allocated']
    for sid in sids:
        pool.close(sid)
