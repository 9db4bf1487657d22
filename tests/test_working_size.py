"""CPU tests around the working-size option (csrc/native_size.hip, ops.masks_to_native, Tracker / StreamPool / Parameters / evaluate.py):
the C ABI and ISA of the new file, the argument checks (they run before any launch, so without a GPU), the wrappers' refusals, the
planners, the configuration, and the fp64 definition of tests/_native_refs.py against torch.  The kernels and the plumbing are checked on
the GPU (tests/test_working_size_gpu.py)."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _native_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
ENTRY_POINTS = ['frtm_masks_to_native', 'frtm_resize_label_map_u8']
FRTM_ERR_ARG = -1


def test_abi_has_the_native_size_entry_points():
    from frtm_vos_amd import _hip, build, ops
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read(), flags=re.S)
    L = _hip.lib()
    for name in ENTRY_POINTS:
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _hip.SIGNATURES and hasattr(L, name), name
    assert 'native_size.hip' in build.SOURCES
    assert ops.MAX_MERGE_OBJECTS + 1 == 16 and ops.MAX_NATIVE_DIM == 16384


def test_native_size_kernels_spill_nothing():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'native_size.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'native_size.hip')], check=True, capture_output=True, cwd=d)
        isa = open(out).read()
    code, meta = isa[:isa.index('amdhsa.kernels:')], isa[isa.index('amdhsa.kernels:'):]
    blocks = [b for b in meta.split('\n  - ') if re.search(r'\.name:\s+_Z\d+k_(masks_to_native|resize_label_map)', b)]
    assert len(blocks) == 2
    for b in blocks:
        for field in ('vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size'):
            assert int(re.search(r'\.%s:\s+(\d+)' % field, b).group(1)) == 0, field
    assert 'ds_write' in code and 'ds_read' in code                   # the LDS patch
    assert 'flat_load' not in code and 'scratch_' not in code and 'atomic' not in code


def _table(rows):
    return (ctypes.c_longlong * (len(rows[0]) * len(rows)))(*[int(v) for r in rows for v in r])


def test_bad_arguments_are_refused_before_any_launch():
    """Every refusal happens on the host from the host copy of the table: no device is needed (or touched) to get FRTM_ERR_ARG."""
    from frtm_vos_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_ubyte * 4096)()
    p = ctypes.addressof(buf)                                     # stands in for the device pointers: nothing dereferences them
    ok = [(0, 2, 9, 13, 0, 0, 0)]

    def native(rows, n=None, h=5, w=7, masks=p, host=True, dev=p, labels=p, soft=p, luts=p):
        t = _table(rows)
        return L.frtm_masks_to_native(masks, 1024, h, w, ctypes.addressof(t) if host else None, dev, len(rows) if n is None else n,
                                      labels, 4096, soft, 1024, luts, 64, None)
    for rows in ([(0, 0, 9, 13, 0, 0, 0)], [(0, 17, 9, 13, 0, -1, 0)], [(0, -1, 9, 13, 0, 0, 0)], [(0, 2, 0, 13, 0, 0, 0)], [(0, 2, 9, 0, 0, 0, 0)],
                 [(0, 2, 16385, 1, 0, -1, 0)], [(0, 2, 1, 16385, 0, -1, 0)], ok + [(70, 17, 9, 13, 200, -1, 2)]):
        assert native(rows) == FRTM_ERR_ARG, rows
        assert b'frtm_masks_to_native' in L.frtm_last_error()
    for kw in (dict(h=0), dict(w=0), dict(h=16385), dict(w=-2), dict(n=0), dict(n=70000), dict(masks=None), dict(host=False), dict(dev=None),
               dict(labels=None), dict(luts=None), dict(soft=None)):                     # (soft NULL while the row asks for planes)
        assert native(ok, **kw) == FRTM_ERR_ARG, kw

    def label_map(rows, n=None, H=30, W=51, nbytes=4096, src=p, out=p, host=True, dev=p):
        t = _table(rows)
        return L.frtm_resize_label_map_u8(src, nbytes, ctypes.addressof(t) if host else None, dev, len(rows) if n is None else n, out, H, W, None)
    for rows in ([(0, 0, 20, 0)], [(0, 10, 0, 0)], [(0, 10, 20, 1)], [(0, 16385, 1, 0)], [(-1, 10, 20, 0)], [(4096 - 199, 10, 20, 0)]):
        assert label_map(rows) == FRTM_ERR_ARG, rows
        assert b'frtm_resize_label_map_u8' in L.frtm_last_error()
    for kw in (dict(H=0), dict(W=0), dict(H=16385), dict(n=0), dict(src=None), dict(out=None), dict(host=False), dict(dev=None), dict(nbytes=199)):
        assert label_map([(0, 10, 20, 0)], **kw) == FRTM_ERR_ARG, kw


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from frtm_vos_amd import ops
    table = ops.NativeTable.packed((5, 7), [(2, 9, 13)], 'cpu')
    assert table.rows.tolist() == [[0, 2, 9, 13, 0, 0, 0]] and (table.label_bytes, table.soft_elems, table.lut_bytes) == (117, 234, 2)
    two = ops.NativeTable.packed((5, 7), [(2, 9, 13), (3, 4, 6)], 'cpu', soft=False)
    assert two.rows.tolist() == [[0, 2, 9, 13, 0, -1, 0], [70, 3, 4, 6, 117, -1, 2]] and (two.label_bytes, two.soft_elems, two.lut_bytes) == (141, 0, 5)
    masks, labels, luts, soft = torch.zeros(2, 5, 7), torch.zeros(117, dtype=torch.uint8), torch.zeros(2, dtype=torch.uint8), torch.zeros(234)
    with pytest.raises(ValueError, match='17 planes'):
        ops.NativeTable.packed((5, 7), [(17, 9, 13)], 'cpu')                              # K = 17
    with pytest.raises(ValueError, match='native size'):
        ops.NativeTable.packed((5, 7), [(2, 16385, 13)], 'cpu')
    with pytest.raises(ValueError, match='native size'):
        ops.NativeTable.packed((5, 7), [(2, 9, 0)], 'cpu')
    with pytest.raises(TypeError):
        ops.masks_to_native(masks.double(), table, labels, luts, soft=soft)             # dtype
    with pytest.raises(TypeError):
        ops.masks_to_native(masks, table, labels.float(), luts, soft=soft)
    with pytest.raises(TypeError):
        ops.masks_to_native(masks, table.rows, labels, luts, soft=soft)
    with pytest.raises(ValueError):
        ops.masks_to_native(masks.view(-1), table, labels, luts, soft=soft)             # rank
    with pytest.raises(ValueError):
        ops.masks_to_native(masks, table, labels.view(9, 13), luts, soft=soft)
    with pytest.raises(ValueError, match='working size'):
        ops.masks_to_native(torch.zeros(1, 1, 16385), table, labels, luts, soft=soft)   # size 16385
    with pytest.raises(ValueError, match='soft'):
        ops.masks_to_native(masks, table, labels, luts)                                 # the table asks for planes
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.masks_to_native(masks, table, labels, luts, soft=soft)
    desc = torch.tensor([[0, 10, 20, 0]])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.resize_label_map_u8(torch.zeros(200, dtype=torch.uint8), desc, (30, 51))
    plan = ops.ResizePlan(desc, 'cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        plan.label_map(torch.zeros(200, dtype=torch.uint8), (30, 51))
    with pytest.raises(TypeError):
        ops.ResizePlan(desc.int(), 'cpu')


def test_planners_put_all_sizes_into_one_batch_under_a_working_size():
    from frtm_vos_amd.model.stream_pool import plan_tick, plan_tick_ragged
    entries = [(0, (128, 160), 1, True), (1, (256, 320), 2, True), (2, (120, 200), 2, True), (3, (256, 320), 1, False), (4, (64, 64), 0, True)]
    for planner in (plan_tick, plan_tick_ragged):
        assert len(planner(entries).batches) == 3                     # one batch per frame size without the option
        assert planner(entries, working_size=None) == planner(entries)
        plan = planner(entries, working_size=(128, 160))
        assert len(plan.batches) == 1 and plan.skipped == [4]
        tb = plan.batches[0]
        assert tb.size == (128, 160) and tb.order == [0, 1, 2, 3] and tb.fallbacks == [3]
        assert plan == planner(entries[::-1], working_size=(128, 160))
    assert plan_tick(entries, working_size=(128, 160)).batches[0].groups == [(0, 1, 1), (1, 2, 2)]
    assert plan_tick_ragged(entries, working_size=(128, 160)).batches[0].groups == [(0, 3, (1, 2, 2))]


def test_the_option_is_off_by_default_everywhere():
    from frtm_vos_amd.evaluate import Parameters, parameters_from_args, parse_args
    from frtm_vos_amd.model.stream_pool import StreamPool
    from frtm_vos_amd.model.tracker import Tracker
    assert Parameters().working_size is None and Parameters(working_size=[480, 854]).working_size == (480, 854)
    assert inspect.signature(Tracker.__init__).parameters['working_size'].default is None
    assert inspect.signature(Tracker.__init__).parameters['working_size'].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert list(inspect.signature(Tracker.__init__).parameters)[-1] == 'working_size'   # after every argument a positional caller passes
    assert inspect.signature(StreamPool.__init__).parameters['working_size'].default is None
    sig = inspect.signature(Parameters.get_stream_pool).parameters
    assert sig['working_size'].default is None and sig['max_streams'].default == 8
    base = ['--model', 'm.pth', '--dset', 'dv2017val', '--dev', 'cpu']
    assert parse_args(base).working_size is None
    args = parse_args(base + ['--working-size', '480', '854'])
    assert args.working_size == (480, 854)
    assert parameters_from_args(args, None).working_size == (480, 854) and parameters_from_args(parse_args(base), None).working_size is None
    with pytest.raises(SystemExit):
        parse_args(base + ['--working-size', '480'])


def test_tracker_refuses_a_bad_working_size():
    from frtm_vos_amd.model.tracker import Tracker
    for bad in ((0, 10), (480, 16385)):
        with pytest.raises(ValueError, match='working_size'):
            Tracker(None, None, None, None, 'cpu', working_size=bad)                    # (refused before any module is touched)


# ---- the definition ----
@pytest.mark.parametrize('planes,size,native', R.SHAPES)
def test_definition_agrees_with_torch(planes, size, native):
    """The fp64 sum over the fp32 taps against F.interpolate(bilinear, align_corners=False), and the decode of both.  The definition's
    taps are fp32 quantities: the source coordinate scale * (d + .5) - .5 carries the rounding of the scale, of the product and of the
    difference, at most 3 * 2^-24 * max(h, w) in all, and the sample moves by at most that per axis on values in [0, 1].  Torch in fp64 has
    the exact coordinate; torch in fp32 rounds its own way (its CPU kernel does not form the coordinate like the device code), within the
    same bound.  The three decodes agree outside the band the GPU tests exclude; the band is under its cap of 1 % everywhere and holds no
    pixel at all of the first six shapes (at the 5x reduction of the first chunk-loop shape a native pixel can sit exactly between two source pixels: 3 of its 1400 pixels do,
    between two objects with equal saturated masks, an exact tie of two planes)."""
    m = R.merged(planes, size[0], size[1], planes * 100 + size[0])
    assert tuple(m.shape) == (planes,) + size and int((m > 0).sum(0).max()) == 1 and float(m.max()) <= 1      # merged: one plane per pixel
    ref = R.native_planes(m, native)
    t64 = F.interpolate(m.double()[None], native, mode='bilinear', align_corners=False)[0]
    t32 = F.interpolate(m[None], native, mode='bilinear', align_corners=False)[0]
    bound = 2 * 3 * 2.0 ** -24 * max(size)
    err64, err32 = float((t64 - ref).abs().max()), float((t32.double() - ref).abs().max())
    lab, margin = R.decode(ref)
    excluded = margin <= R.LABEL_MARGIN
    print(planes, size, native, 'max |torch fp64 - def| %.2e, |torch fp32 - def| %.2e, bound %.2e, excluded %d, labels'
          % (err64, err32, bound, int(excluded.sum())), lab.unique().tolist())
    assert err64 <= bound and err32 <= bound + R.SOFT_TOL
    assert float(excluded.float().mean()) <= R.EXCLUDED_CAP
    if (planes, size, native) in R.SHAPES[:6]:
        assert int(excluded.sum()) == 0
    assert bool(((lab == R.decode(t64)[0]) | excluded).all()) and bool(((lab == R.decode(t32.double())[0]) | excluded).all())
    if size == native:
        assert torch.equal(ref, m.double())


def test_nearest_index_is_torchs():
    for src, dst in ((37, 12), (53, 20), (5, 11), (3, 9), (7, 7), (1080, 480)):
        ids = torch.arange(src, dtype=torch.float32).view(1, 1, 1, src)
        assert np.array_equal(F.interpolate(ids, (1, dst), mode='nearest')[0, 0, 0].numpy().astype(np.int64), R.nearest_index(src, dst))
