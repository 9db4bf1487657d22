"""StreamPool and grouped target-model scoring without a GPU: the C ABI of frtm_target_apply_grouped, the tick planner (a pure function),
the pool's refusals, and the unchanged defaults of the training entry points."""
import inspect
import os
import random
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_declares_exports_and_binds_the_new_symbol():
    import ctypes
    from frtm_vos_amd import _hip, build, ops
    hdr = open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read()
    name = 'frtm_target_apply_grouped'
    assert re.search(r'\b%s\s*\(' % name, hdr) and name in _hip.SIGNATURES and hasattr(_hip.lib(), name)
    res, args = _hip.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == 14 and args[1] is ctypes.c_size_t          # (the frame pitch is a size_t)
    assert 'target_apply_grouped.hip' in build.SOURCES
    assert callable(ops.target_apply_grouped)


def test_entry_refuses_unsupported_shapes_with_a_message():
    """The argument checks run before anything touches the device: c = 160, Cin not a multiple of the K chunk, a pitch below a frame."""
    from frtm_vos_amd import _hip
    L = _hip.lib()
    one = 0x1000          # a non-null address the checks never dereference
    for Cin, c, pitch, word in ((256, 160, 256 * 80, b'128'), (100, 96, 100 * 80, b'multiple'), (256, 96, 17, b'pitch')):
        rc = L.frtm_target_apply_grouped(one, pitch, 1, one, one, one, 1, Cin, c, 8, 10, one, one, None)
        assert rc == -1 and word in L.frtm_last_error(), (Cin, c, pitch, L.frtm_last_error())


ENTRIES = [(4, (128, 160), 2, True), (0, (128, 160), 2, True), (7, (128, 160), 1, True), (2, (128, 160), 3, False), (5, (64, 96), 2, True),
           (3, (128, 160), 2, True), (6, (128, 160), 0, False), (1, (64, 96), 1, False)]


def test_planner_groups_by_size_and_object_count():
    from frtm_vos_amd.model.stream_pool import plan_tick
    plan = plan_tick(ENTRIES)
    assert plan.skipped == [6]                                             # no active object: takes no part
    assert [b.size for b in plan.batches] == [(64, 96), (128, 160)]        # mixed sizes: separate trunk batches
    small, big = plan.batches
    assert small.order == [5, 1] and small.groups == [(0, 1, 2)] and small.fallbacks == [1]
    assert big.order == [7, 0, 3, 4, 2]
    assert big.groups == [(0, 1, 1), (1, 3, 2)]                            # streams of one object count are adjacent: one slice of the taps
    assert big.fallbacks == [4]                                            # the ineligible stream runs its own track()
    for b in plan.batches:
        covered = sorted([k for s, g, _ in b.groups for k in range(s, s + g)] + b.fallbacks)
        assert covered == list(range(len(b.order)))                        # every stream of the batch exactly once
        n_of = {sid: n for sid, _, n, _ in ENTRIES}
        for s, g, n in b.groups:
            assert all(n_of[sid] == n for sid in b.order[s:s + g])


def test_planner_does_not_depend_on_dict_order():
    from frtm_vos_amd.model.stream_pool import plan_tick
    ref = plan_tick(ENTRIES)
    rng = random.Random(3)
    for _ in range(20):
        e = list(ENTRIES)
        rng.shuffle(e)
        assert plan_tick(e) == ref
    assert plan_tick([]) == plan_tick(iter(())) and plan_tick([]).batches == []


def _stub_pool(**kw):
    from frtm_vos_amd.evaluate import AttrDict
    from frtm_vos_amd.model.stream_pool import StreamPool
    aug = types.SimpleNamespace(augment_first_frame=lambda image, mask: (image, mask))
    return StreamPool(aug, None, AttrDict(update_filters=True), torch.nn.Identity(), kw.pop('device', 'cuda:0'), **kw)


def test_pool_refusals():
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _stub_pool(device='cpu')
    pool = _stub_pool(max_streams=2)
    a, b = pool.open(), pool.open()
    assert a != b and len(pool) == 2
    with pytest.raises(RuntimeError, match='max_streams'):
        pool.open()
    with pytest.raises(KeyError):
        pool.close(99)
    with pytest.raises(KeyError):
        pool.step({99: torch.zeros(3, 8, 8, dtype=torch.uint8)})
    with pytest.raises(KeyError):
        pool.initialize(99, None, None, [])
    pool.close(a)
    c = pool.open()                                                        # a closed stream's place is free again; ids are not reused
    assert c not in (a, b) and len(pool) == 2
    assert pool.step({}) == {}


def test_pool_streams_share_the_modules_and_the_target_model_pool():
    pool = _stub_pool(max_streams=3)
    t0, t1 = pool.tracker(pool.open()), pool.tracker(pool.open())
    assert t0 is not t1 and t0.refiner is t1.refiner is pool.refiner and t0.augmenter is t1.augmenter
    assert t0._disc_pool is t1._disc_pool is pool._disc_pool
    assert pool.min_pairs >= 1 and pool.grouped_apply in (True, False)


def test_training_defaults_are_unchanged():
    from frtm_vos_amd.model.training_model import TargetModelBank, TrainerModel
    from frtm_vos_amd.train import ModelParameters, parse_args
    assert inspect.signature(TargetModelBank.scores).parameters['grouped'].default is False
    assert inspect.signature(TrainerModel.__init__).parameters['batched_scores'].default is False
    assert inspect.signature(ModelParameters.__init__).parameters['batched_scores'].default is False
    assert parse_args(['x']).batched_scores is False and parse_args(['x', '--batched-scores']).batched_scores is True
    from frtm_vos_amd.evaluate import Parameters
    sig = inspect.signature(Parameters.get_stream_pool).parameters
    assert sig['max_streams'].default == 8
