"""Ragged StreamPool groups without a GPU: the C ABI of csrc/ragged_group.hip, the ragged tick planner (a pure function), the
sample-to-frame table, the refusals of the four indexed wrappers, forward_torch with a table against per-frame calls, and the defaults."""
import inspect
import os
import random
import re
from collections import OrderedDict

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('frtm_tse_inject_indexed', 'frtm_cab_gate_indexed', 'frtm_cab_combine_indexed', 'frtm_track_merge_ragged')

# the entries of tests/test_stream_pool.py: (sid, frame size, active objects, eligible)
ENTRIES = [(4, (128, 160), 2, True), (0, (128, 160), 2, True), (7, (128, 160), 1, True), (2, (128, 160), 3, False), (5, (64, 96), 2, True),
           (3, (128, 160), 2, True), (6, (128, 160), 0, False), (1, (64, 96), 1, False)]


def test_abi_declares_exports_and_binds_the_four_entry_points():
    import ctypes
    from frtm_vos_amd import _hip, build, ops
    hdr = open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read()
    for name in NAMES:
        assert re.search(r'\bint %s\s*\(' % name, hdr), name
        assert name in _hip.SIGNATURES and hasattr(_hip.lib(), name), name
        res, args = _hip.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(re.search(r'\bint %s\s*\(([^)]*)\)' % name, hdr).group(1).split(',')), name
    assert 'ragged_group.hip' in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'ragged_group.hip'))
    for fn in ('tse_inject_indexed', 'cab_gate_indexed', 'cab_combine_indexed', 'track_merge_ragged', 'RaggedTable'):
        assert callable(getattr(ops, fn)), fn


def test_entry_points_refuse_sizes_and_grids_with_a_message():
    """The host-side checks of the twins: empty maps, samples beyond the grid, oc no multiple of 4, the LDS bound of the gate, no frame."""
    from frtm_vos_amd import _hip
    L = _hip.lib()
    one = 0x1000          # a non-null address the checks never dereference
    assert L.frtm_tse_inject_indexed(one, one, one, one, 2, one, 1, 4, 0, 5, 8, 8, one, None) == -1 and b'positive' in L.frtm_last_error()
    assert L.frtm_tse_inject_indexed(one, one, one, one, 16384, one, 1, 4, 4, 4, 8, 8, one, None) == -1 and b'samples per call' in L.frtm_last_error()
    assert L.frtm_tse_inject_indexed(one, one, one, one, 2, one, 0, 4, 4, 4, 8, 8, one, None) == -1 and b'bad argument' in L.frtm_last_error()
    assert L.frtm_cab_gate_indexed(one, one, one, 1, one, one, one, one, 2, 6, one, None) == -1 and b'multiple of 4' in L.frtm_last_error()
    assert L.frtm_cab_gate_indexed(one, one, one, 1, one, one, one, one, 2, 2344, one, None) == -1 and b'LDS' in L.frtm_last_error()
    assert L.frtm_cab_combine_indexed(one, one, one, one, 1, 2, 4, 1, 0, 8, 8, one, None) == -1 and b'positive' in L.frtm_last_error()
    assert L.frtm_cab_combine_indexed(one, one, one, one, 1, 1024, 64, 1, 1, 8, 8, one, None) == -1 and b'65535 planes' in L.frtm_last_error()
    assert L.frtm_track_merge_ragged(one, 0, one, 64, one, None, 0.5, None) == -1 and b'frames' in L.frtm_last_error()
    assert L.frtm_track_merge_ragged(one, 2, one, 0, one, None, 0.5, None) == -1 and b'bad argument' in L.frtm_last_error()


def test_ragged_planner_on_the_entries_of_the_uniform_planner():
    from frtm_vos_amd.model.stream_pool import plan_tick, plan_tick_ragged
    plan = plan_tick_ragged(ENTRIES)
    assert plan.skipped == [6]
    assert [b.size for b in plan.batches] == [(64, 96), (128, 160)]
    small, big = plan.batches
    assert small.order == [5, 1] and small.groups == [(0, 1, (2,))] and small.fallbacks == [1]
    assert big.order == [7, 0, 3, 4, 2] and big.groups == [(0, 4, (1, 2, 2, 2))] and big.fallbacks == [4]
    uniform = plan_tick(ENTRIES)                                           # the same batches, order, fallbacks and skipped streams
    assert uniform.skipped == plan.skipped
    assert [(b.size, b.order, b.fallbacks) for b in uniform.batches] == [(b.size, b.order, b.fallbacks) for b in plan.batches]


def test_ragged_planner_properties():
    from frtm_vos_amd.model.stream_pool import plan_tick_ragged
    ref = plan_tick_ragged(ENTRIES)
    rng = random.Random(3)
    for _ in range(20):
        e = list(ENTRIES)
        rng.shuffle(e)
        assert plan_tick_ragged(e) == ref
    assert plan_tick_ragged([]) == plan_tick_ragged(iter(())) and plan_tick_ragged([]).batches == []
    many = ENTRIES + [(9, (128, 160), 16, True), (8, (128, 160), 15, True)]
    plan = plan_tick_ragged(many)
    n_of = {sid: n for sid, _, n, _ in many}
    for b in plan.batches:
        assert len(b.groups) <= 1                                          # one group per frame size
        covered = sorted([k for s, g, _ in b.groups for k in range(s, s + g)] + b.fallbacks)
        assert covered == list(range(len(b.order)))                        # every stream of the batch exactly once
        for s, g, counts in b.groups:
            assert len(counts) == g and [n_of[sid] for sid in b.order[s:s + g]] == list(counts) == sorted(counts)
    big = plan.batches[1]
    assert big.groups == [(0, 5, (1, 2, 2, 2, 15))]
    assert big.order.index(9) in big.fallbacks                             # 16 objects: beyond the merge kernel, its own track()
    assert big.order[big.fallbacks[0]:] == [2, 9]                          # fallbacks by sid


def test_ragged_table_on_the_cpu():
    from frtm_vos_amd import ops
    t = ops.RaggedTable((3, 1, 2), 'cpu')
    assert t.counts == (3, 1, 2) and t.F == 3 and t.n == 6
    assert t.frame_of.dtype == torch.int32 and t.frame_of.tolist() == [0, 0, 0, 1, 2, 2]
    assert t.first.dtype == torch.int32 and t.first.tolist() == [0, 3, 4, 6]
    assert [t.planes(f) for f in range(3)] == [(0, 4), (4, 6), (6, 9)]     # n_f + 1 packed planes per frame
    for bad in ((), (0,), (16,), (2, 0, 1), (3, 16)):
        with pytest.raises(ValueError, match='RaggedTable'):
            ops.RaggedTable(bad, 'cpu')
    assert ops.RaggedTable((15,), 'cpu').n == 15


def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


def _wrapper_cases():
    """name -> (a call with the arguments given by keyword overrides, the good arguments): all CPU tensors, table (3, 1, 2)."""
    from frtm_vos_amd import ops
    t = ops.RaggedTable((3, 1, 2), 'cpu')
    return {
        'tse_inject_indexed': (lambda base, bias, ws, scores: ops.tse_inject_indexed(base, bias, ws, scores, t),
                               dict(base=_z(3, 4, 8, 8), bias=_z(4), ws=_z(4, 9), scores=_z(6, 1, 4, 4))),
        'cab_gate_indexed': (lambda sp, dp, w1t, b1, w2t, b2: ops.cab_gate_indexed(sp, dp, w1t, b1, w2t, b2, t),
                             dict(sp=_z(6, 8), dp=_z(3, 8), w1t=_z(16, 8), b1=_z(8), w2t=_z(8, 8), b2=_z(8))),
        'cab_combine_indexed': (lambda shallow, gate, deeper: ops.cab_combine_indexed(shallow, gate, deeper, t),
                                dict(shallow=_z(6, 4, 8, 8), gate=_z(6, 4), deeper=_z(3, 4))),
        'track_merge_ragged': (lambda logits, masks, counts: ops.track_merge_ragged(logits, t, masks, counts),
                               dict(logits=_z(6, 1, 8, 8), masks=_z(9, 8, 8), counts=_z(9, dtype=torch.int32))),
    }


BAD_SHAPES = {
    'tse_inject_indexed': [dict(scores=_z(5, 1, 4, 4)), dict(base=_z(2, 4, 8, 8)), dict(bias=_z(5)), dict(scores=_z(6, 4, 4))],
    'cab_gate_indexed': [dict(sp=_z(5, 8)), dict(dp=_z(6, 8)), dict(dp=_z(3, 12)), dict(sp=_z(6, 8, 1))],
    'cab_combine_indexed': [dict(shallow=_z(5, 4, 8, 8), gate=_z(5, 4)), dict(deeper=_z(6, 4)), dict(deeper=_z(3, 5)), dict(shallow=_z(6, 4, 64))],
    'track_merge_ragged': [dict(logits=_z(5, 1, 8, 8)), dict(masks=_z(6, 8, 8)), dict(counts=_z(6, dtype=torch.int32)), dict(masks=_z(3, 3, 8, 8))],
}
BAD_DTYPES = {
    'tse_inject_indexed': dict(scores=_z(6, 1, 4, 4, dtype=torch.float64)),
    'cab_gate_indexed': dict(dp=_z(3, 8, dtype=torch.float16)),
    'cab_combine_indexed': dict(gate=_z(6, 4, dtype=torch.float64)),
    'track_merge_ragged': dict(counts=_z(9, dtype=torch.int64)),
}


@pytest.mark.parametrize('name', list(BAD_SHAPES))
def test_wrapper_refusals_need_no_device(name):
    call, good = _wrapper_cases()[name]
    for bad in BAD_SHAPES[name]:
        with pytest.raises(ValueError, match='^%s: ' % name):
            call(**dict(good, **bad))
    with pytest.raises(TypeError, match='^%s: ' % name):
        call(**dict(good, **BAD_DTYPES[name]))
    if name == 'track_merge_ragged':
        with pytest.raises(TypeError, match='^track_merge_ragged: '):
            call(**dict(good, logits=_z(6, 1, 8, 8, dtype=torch.float64)))


def _close(a, b, what):
    """The rule of tests/test_refiner_kernels.py::_close."""
    e, m = float((a - b).abs().max()), float(b.abs().max())
    assert a.shape == b.shape and e <= 1e-12 * m, '%s: err %.3e, max|ref| %.3e' % (what, e, m)


def test_forward_torch_with_a_table_equals_the_per_frame_calls():
    from frtm_vos_amd import ops
    from frtm_vos_amd.model.seg_network import SegNetwork
    chans = OrderedDict(layer5=40, layer4=24, layer3=16, layer2=8)
    torch.manual_seed(5)
    net = SegNetwork(1, 8, chans).eval().double()
    size, counts = (96, 140), (1, 3, 2)
    table = ops.RaggedTable(counts, 'cpu')
    g = torch.Generator().manual_seed(19)
    dims = [((size[0] + 2 ** k - 1) // 2 ** k, (size[1] + 2 ** k - 1) // 2 ** k) for k in (5, 4, 3, 2)]
    feats = {L: torch.relu(torch.randn(3, c, *d, generator=g)).double() for (L, c), d in zip(chans.items(), dims)}
    scores = torch.randn(table.n, 1, *dims[1], generator=g).double()
    with torch.no_grad():
        got = net.forward_torch(scores, feats, size, frame_of=table)
        assert torch.equal(net(scores, feats, size, frame_of=table), got)                   # forward on CPU tensors is forward_torch
        parts = [net.forward_torch(scores[table.starts[f]:table.starts[f + 1]], {L: t[f:f + 1] for L, t in feats.items()}, size)
                 for f in range(3)]
    ref = torch.cat(parts)
    assert tuple(got.shape) == (6, 1) + size and float(ref.abs().max()) > 1e-3
    _close(got, ref, 'forward_torch with counts %r' % (counts,))
    assert not torch.equal(parts[1][0], parts[1][1])                                       # (the objects of a frame differ)
    with pytest.raises(ValueError, match='table'):
        net(scores[:5], feats, size, frame_of=table)


def test_defaults_are_off():
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.model.seg_network import SegNetwork
    from frtm_vos_amd.model.stream_pool import StreamPool
    from frtm_vos_amd.model.tracker import fused_step
    assert inspect.signature(StreamPool.__init__).parameters['ragged_groups'].default is False
    assert inspect.signature(Parameters.get_stream_pool).parameters['ragged_groups'].default is False
    assert inspect.signature(SegNetwork.forward).parameters['frame_of'].default is None
    assert inspect.signature(SegNetwork.forward_torch).parameters['frame_of'].default is None
    assert inspect.signature(fused_step).parameters['table'].default is None
