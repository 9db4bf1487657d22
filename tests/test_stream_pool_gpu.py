"""Grouped target-model scoring (csrc/target_apply_grouped.hip) and StreamPool (model/stream_pool.py) on the GPU.

Kernel level, against fp64.  Every projected feature is one chain of Cin fused multiply-adds and every score a sum of 9c products:
a sum of n terms, each rounded once per operation in any order, is off by at most gamma(n) * sum |a_i b_i| with
gamma(n) = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  Hence

    |cft - cft64| <= gamma(Cin + 1) * (|W|^T |X|)
    |s - s64|     <= gamma(9c + 1) * (|f| conv |cft|)  +  |f| conv (gamma(Cin + 1) * |W|^T |X|)

the second line being the rounding of the 3x3 pass over the features the kernel really read plus the projection's own error carried
through the filter (both bounds: tests/_grouped_refs.py, shared with tests/test_grouped_scoring_gpu.py, which runs the kernels' other tile
forms and edges).  A mixed-up pair, frame or table entry misses these bounds by orders of magnitude (the data is O(1), the bounds 1e-5).
Pairs do not interact, so a pair's result must be BITWISE the same alone, inside a larger launch and with the tables reversed.

Pool level: four streams against one fresh Tracker per stream running the reference's literal loop, with the gates of
tests/test_fullsize_gpu.py::test_run_sequence_matches_the_literal_per_frame_loop; run-to-run equality; no device allocation in steady state."""
import types

import pytest
import torch

from _grouped_refs import _bounds, _worst

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = 'cuda'


# (Cin, c, h, w, frames, frame_of_pair, extra floats between frames)
CASES = {
    'shared-frames': (256, 96, 8, 10, 3, [0, 0, 1, 2, 2], 0),        # h*w = 80: no multiple of the column tile; c = 96: no multiple of 64
    'one-pair-pitched': (256, 96, 5, 7, 2, [1], 1000),               # G = 1, the frames not dense
    'product-shape': (1024, 96, 30, 54, 2, [0, 1, 1], 0),            # RN101 at 480p: 26 column tiles, 32 K chunks
}


def _make(name):
    Cin, c, h, w, frames, fop, extra = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    store = torch.randn(frames, Cin * h * w + extra, generator=g).relu()           # ReLU'd normal features
    w1T = [torch.randn(Cin, c, generator=g) / Cin ** 0.5 for _ in fop]             # distinct weights per pair, GEMM layout [Cin][c]
    w2 = [torch.randn(1, c, 3, 3, generator=g) / (9 * c) ** 0.5 for _ in fop]
    return types.SimpleNamespace(Cin=Cin, c=c, h=h, w=w, frames=frames, fop=fop, store=store, w1T=w1T, w2=w2,
                                 X=store[:, :Cin * h * w].reshape(frames, Cin, h, w))


def _run(case, pairs):
    """The kernel on the pairs ``pairs`` (indices into the case's tables, in this order) -> (cft, scores) on the host."""
    from frtm_vos_amd import ops
    store = case.store.to(DEV)
    feats = store[:, :case.Cin * case.h * case.w].view(case.frames, case.Cin, case.h, case.w)
    assert case.frames == 1 or feats.stride(0) == store.shape[1]
    w1T = [case.w1T[p].to(DEV) for p in pairs]
    w2 = [case.w2[p].to(DEV) for p in pairs]
    fop = torch.tensor([case.fop[p] for p in pairs], dtype=torch.int32, device=DEV)
    cft, s = ops.target_apply_grouped(feats, fop, ops.pointer_table(w1T, DEV), ops.pointer_table(w2, DEV), case.c)
    torch.cuda.synchronize()
    assert tuple(cft.shape) == (len(pairs), case.c, case.h, case.w) and tuple(s.shape) == (len(pairs), 1, case.h, case.w)
    return cft.cpu(), s.cpu()


@pytest.mark.parametrize('name', list(CASES))
def test_grouped_apply_against_fp64(name):
    case = _make(name)
    cft, s = _run(case, list(range(len(case.fop))))
    assert bool(torch.isfinite(cft).all()) and bool(torch.isfinite(s).all())
    worst = [0.0, 0.0]
    for p, f in enumerate(case.fop):
        cft64, b1, s64, b2 = _bounds(case.Cin, case.c, case.X[f], case.w1T[p], case.w2[p], cft[p])
        worst[0] = max(worst[0], _worst(cft[p], cft64, b1))
        worst[1] = max(worst[1], _worst(s[p], s64, b2))
        assert float(cft64.abs().max()) > 0.5 and float(s64.abs().max()) > 0.05      # (the data is O(1): the bounds mean something)
    print('%s: worst error / bound: projection %.2e, scores %.2e' % (name, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


def test_a_pairs_result_does_not_depend_on_the_launch():
    """Pair p alone (G = 1), inside the G = 5 launch and with the table order reversed: bitwise the same projected features and scores."""
    case = _make('shared-frames')
    G = len(case.fop)
    cft, s = _run(case, list(range(G)))
    cft_r, s_r = _run(case, list(range(G - 1, -1, -1)))
    for p in range(G):
        cft_1, s_1 = _run(case, [p])
        assert torch.equal(cft_1[0], cft[p]) and torch.equal(s_1[0], s[p]), p
        assert torch.equal(cft_r[G - 1 - p], cft[p]) and torch.equal(s_r[G - 1 - p], s[p]), p
    assert not torch.equal(cft[0], cft[1])                                             # (pairs 0 and 1 share a frame, not their weights)


def test_the_product_shape_is_bitwise_the_same_under_both_column_tiles():
    """G = 3 at 30x54 takes the 32-column tile, G = 12 the 64-column one (26 x 12 >= 256 workgroups): the same chain per element."""
    case = _make('product-shape')
    cft, s = _run(case, [0, 1, 2])
    cft_12, s_12 = _run(case, [0, 1, 2] * 4)
    for r in range(4):
        assert torch.equal(cft_12[3 * r:3 * r + 3], cft) and torch.equal(s_12[3 * r:3 * r + 3], s)


def test_unsupported_shapes_raise():
    from frtm_vos_amd import ops
    feats = torch.randn(1, 256, 8, 10, device=DEV).relu()
    fop = torch.zeros(1, dtype=torch.int32, device=DEV)
    w1T, w2 = [torch.randn(256, 160, device=DEV)], [torch.randn(1, 160, 3, 3, device=DEV)]
    with pytest.raises(RuntimeError, match='128'):
        ops.target_apply_grouped(feats, fop, ops.pointer_table(w1T, DEV), ops.pointer_table(w2, DEV), 160)
    with pytest.raises(RuntimeError, match='multiple'):
        ops.target_apply_grouped(feats[:, :100].contiguous(), fop, ops.pointer_table(w1T, DEV), ops.pointer_table(w2, DEV), 96)
    with pytest.raises(ValueError):
        ops.target_apply_grouped(feats.cpu(), fop, ops.pointer_table(w1T, DEV), ops.pointer_table(w2, DEV), 96)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------------------
# the pool against the literal loop
# ----------------------------------------------------------------------------------------------------------------------------------
SIZE = (128, 160)


def _params():
    from frtm_vos_amd.evaluate import Parameters
    torch.manual_seed(0)
    params = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18', feature_batch=8, trunk_lanes=2)
    params.disc_params.update(memory_size=8, init_iters=(2, 3), update_iters=(3,))
    return params


@pytest.fixture(scope='module')
def sequences():
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    seqs = [SyntheticSequence('a', 12, SIZE, 2, seed=9), SyntheticSequence('b', 12, SIZE, 2, seed=10),
            SyntheticSequence('c', 11, SIZE, 1, seed=11),                              # one frame shorter: closed while the others go on
            SyntheticSequence('d', 12, SIZE, 3, seed=12, late_object_at=5)]           # falls back on frame 5, joins a group after it
    for s in seqs:
        s.preload(DEV)
    return seqs


def _literal_loop(seq):
    """One fresh Tracker running the reference's loop (tracker.py:130-157): initialize(), then track(image) frame by frame."""
    trk = _params().get_model().eval()
    soft = {}
    for i, (image, labels, new_objects) in enumerate(seq):
        had = len(trk.targets) > 0
        if len(new_objects) > 0:
            torch.manual_seed(0)                     # every target model starts from the same draw, in the pool as here
            trk.initialize(image.to(DEV), labels.to(DEV), new_objects)
        if had:
            soft[i] = trk.track(image.to(DEV)).clone()
        trk.current_frame += 1
    torch.cuda.synchronize()
    return soft


def _pool_run(seqs, grouped):
    pool = _params().get_stream_pool(max_streams=4, grouped_apply=grouped)
    sids = [pool.open() for _ in seqs]
    soft = [dict() for _ in seqs]
    fused = 0
    for t in range(max(len(s) for s in seqs)):
        frames = {}
        for k, seq in enumerate(seqs):
            if t >= len(seq):
                continue
            image, labels, new_objects = seq[t]
            if len(new_objects) > 0:
                torch.manual_seed(0)
                pool.initialize(sids[k], image, labels, new_objects)
            frames[sids[k]] = image
        before = pool.grouped_launches
        out = pool.step(frames)
        fused += pool.grouped_launches - before
        for k, seq in enumerate(seqs):
            if sids[k] in out:
                soft[k][t] = out[sids[k]].clone()
            if t < len(seq):
                assert pool.tracker(sids[k]).current_frame == t + 1
            if t + 1 == len(seq):
                pool.close(sids[k])
    torch.cuda.synchronize()
    assert len(pool) == 0
    return soft, fused


@pytest.fixture(scope='module')
def literal(sequences):
    return [_literal_loop(s) for s in sequences]


@pytest.fixture(scope='module')
def grouped_run(sequences):
    return _pool_run(sequences, True)


def _labels(masks):
    from frtm_vos_amd import ops
    return ops.merge_masks_(masks.clone()).argmax(dim=0)


def _compare(pool_soft, literal):
    for k, (got, ref) in enumerate(zip(pool_soft, literal)):
        assert sorted(got) == sorted(ref) and len(ref) >= 10, (k, sorted(got), sorted(ref))      # the same frames were tracked
        agree = sum(float((_labels(got[t]) == _labels(ref[t])).float().sum()) for t in ref) / sum(ref[t][0].numel() for t in ref)
        d = max(float((got[t] - ref[t]).abs().mean()) for t in ref)
        spread = float(torch.cat([ref[t][1:].reshape(-1) for t in ref]).std())
        print('stream %d: label agreement %.5f, max mean |soft mask diff| %.2e, spread of the object planes %.2e' % (k, agree, d, spread))
        assert agree > 0.995, (k, agree)
        assert d < 2e-3 and spread > 1e-3, (k, d, spread)


def test_pool_with_grouped_apply_matches_the_literal_loop(grouped_run, literal):
    soft, fused = grouped_run
    assert fused > 0                                   # the grouped kernels really ran
    _compare(soft, literal)


def test_pool_with_per_pair_apply_matches_the_literal_loop(sequences, literal):
    soft, fused = _pool_run(sequences, False)
    assert fused == 0
    _compare(soft, literal)


def test_a_pool_of_one_stream_is_bitwise_the_literal_loop(sequences, literal):
    """One stream is a group with g = 1 scored pair by pair: track()'s launches on track()'s shapes, through the same definition of
    the tracking step (model/tracker.py: fused_step).  So no tolerance: the masks of every frame are the literal loop's, bit for bit."""
    soft, fused = _pool_run(sequences[:1], False)
    assert fused == 0 and sorted(soft[0]) == sorted(literal[0]) and len(literal[0]) >= 10
    for t in literal[0]:
        assert torch.equal(soft[0][t], literal[0][t]), t


def test_two_pool_runs_are_bitwise_equal(sequences, grouped_run):
    """No race on the shared tap buffers, the merge buffers or the pointer tables: a second run gives the same masks on every frame."""
    again, _ = _pool_run(sequences, True)
    for a, b in zip(again, grouped_run[0]):
        assert sorted(a) == sorted(b)
        for t in a:
            assert torch.equal(a[t], b[t]), t


def test_steady_ticks_allocate_nothing_on_the_device():
    """The project's invariant (hipMalloc stalls the queue): after the warm-up -- past the first filter re-solve at frame 8 -- four ticks,
    the re-solve of frame 16 among them, ask the driver for no memory.  The counter is the allocator's count of device mallocs
    ('num_device_alloc', what bench.py reports) together with its reserved bytes; 'allocation.all.allocated' also counts every block the
    refiner's torch.empty calls take from the CACHE, which is not a device allocation, and is printed only."""
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    seqs = [SyntheticSequence('m%d' % k, 17, SIZE, 2, seed=20 + k) for k in range(2)]
    for s in seqs:
        s.preload(DEV)
    pool = _params().get_stream_pool(max_streams=2, grouped_apply=True)
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
    st0, n0 = torch.cuda.memory_stats(), pool.grouped_launches
    for t in range(13, 17):
        assert len(tick(t)) == 2
    torch.cuda.synchronize()
    st1 = torch.cuda.memory_stats()
    print('cache allocations over 4 ticks: %d, device mallocs: %d' % (st1['allocation.all.allocated'] - st0['allocation.all.allocated'],
                                                                       st1['num_device_alloc'] - st0['num_device_alloc']))
    assert pool.grouped_launches == n0 + 4             # one grouped launch per tick: both streams in one group
    assert st1['num_device_alloc'] == st0['num_device_alloc']
    assert st1['reserved_bytes.all.allocated'] == st0['reserved_bytes.all.allocated']
    for sid in sids:
        pool.close(sid)


# ----------------------------------------------------------------------------------------------------------------------------------
# the training bank
# ----------------------------------------------------------------------------------------------------------------------------------
def test_bank_scores_grouped_and_per_sample_within_the_fp64_bound():
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.model.training_model import TargetModelBank
    P = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18')
    Cin, c, h, w, B = 256, P.disc_params.c_channels, 8, 10, 3
    bank = TargetModelBank(P.disc_params, B)
    g = torch.Generator().manual_seed(5)
    for slot in bank.slots:
        d = slot.discriminator
        d.project.weight.data.copy_(torch.randn(c, Cin, 1, 1, generator=g) / Cin ** 0.5)
        d.filter.weight.data.copy_(torch.randn(1, c, 3, 3, generator=g) / (9 * c) ** 0.5)
        d._invalidate()
    X = torch.randn(B, Cin, h, w, generator=g).relu()
    per_sample = bank.scores(X.to(DEV)).cpu()
    cfts = [slot.discriminator.current_sample.cpu() for slot in bank.slots]
    grouped = bank.scores(X.to(DEV), grouped=True).cpu()
    cfts_g = [slot.discriminator.current_sample.cpu() for slot in bank.slots]
    assert tuple(grouped.shape) == tuple(per_sample.shape) == (B, 1, h, w)
    assert all(slot.discriminator.frame_num == 2 for slot in bank.slots)
    for i, slot in enumerate(bank.slots):
        d = slot.discriminator
        w1T = d.project.weight.data.view(c, Cin).t().cpu()
        for name, s, cft in (('per sample', per_sample, cfts[i]), ('grouped', grouped, cfts_g[i])):
            cft64, b1, s64, b2 = _bounds(Cin, c, X[i], w1T, d.filter.weight.data.cpu(), cft[0])
            r1, r2 = _worst(cft[0], cft64, b1), _worst(s[i], s64, b2)
            print('slot %d %s: worst error / bound: projection %.2e, scores %.2e' % (i, name, r1, r2))
            assert r1 <= 1.0 and r2 <= 1.0, (i, name, r1, r2)
    again = bank.scores(X.to(DEV), grouped=True).cpu()                                   # (tables and workspace reused)
    assert torch.equal(again, grouped)


def test_trainer_model_forward_with_batched_scores():
    import math
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    from frtm_vos_amd.model.augmenter import ImageAugmenter
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    from frtm_vos_amd.model.seg_network import SegNetwork
    from frtm_vos_amd.model.training_model import SampleSpec, TrainerModel
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    try:
        P = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18')
        P.disc_params.update(memory_size=20, init_iters=(3, 5), update_iters=(3,), c_channels=32)
        ext = ResnetFeatureExtractor('resnet18').to(DEV)
        chans = {L: n for L, n in ext.get_out_channels().items() if L in P.refnet_params.layers}
        torch.manual_seed(1)
        refiner = SegNetwork(1, 64, chans, True).to(DEV)
        seqs = [SyntheticSequence('s%d' % k, 3, SIZE, 1, seed=30 + k) for k in range(2)]
        images = [torch.stack([s.images[t] for s in seqs]) for t in range(3)]
        labels = [torch.stack([(s.gt[t] == 1).to(torch.uint8) for s in seqs]) for t in range(3)]
        meta = [SampleSpec('s%d' % k, 1, ['00000', '00001', '00002'], 0).encoded() for k in range(2)]
        stats = {}
        for batched in (False, True):
            __import__('numpy').random.seed(0)
            torch.manual_seed(0)
            m = TrainerModel(ImageAugmenter(P.aug_params), ext, P.disc_params, refiner, batch_size=2, device=DEV, refiner_backend='hip',
                             loss_backend='hip', batched_scores=batched)
            refiner.zero_grad()
            stats[batched] = m(images, labels, meta)
            assert (m.bank._grouped is not None) == batched
        print('TrainerModel.forward: per sample %r, batched %r' % (stats[False], stats[True]))
        for st in stats.values():
            assert math.isfinite(st['stats/loss']) and math.isfinite(st['stats/accuracy']) and st['stats/loss'] > 0
    finally:
        torch.set_grad_enabled(prev)
