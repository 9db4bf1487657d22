"""CPU tests around csrc/frame_resize.hip: its C ABI and ISA, the argument checks (they run before any launch, so without a GPU), the
wrappers' refusals, and the fp64 restatements of tests/_frame_refs.py against torch wherever torch has the operator.  The kernels
themselves are checked on the GPU (tests/test_frame_resize_gpu.py)."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _frame_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
ENTRY_POINTS = ['frtm_resize_frames_u8', 'frtm_resize_labels_u8']
FRTM_ERR_ARG = -1


def test_abi_has_the_resize_entry_points():
    from frtm_vos_amd import _hip, ops
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read(), flags=re.S)
    L = _hip.lib()
    for name in ENTRY_POINTS:
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _hip.SIGNATURES and hasattr(L, name), name
    for mode, value in ops.RESIZE_MODES.items():
        assert int(re.search(r'#define FRTM_RESIZE_%s (\d+)' % mode.upper(), hdr).group(1)) == value


def test_resize_kernels_spill_nothing_and_stage_with_wide_loads():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'frame_resize.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'frame_resize.hip')], check=True, capture_output=True, cwd=d)
        isa = open(out).read()
    code, meta = isa[:isa.index('amdhsa.kernels:')], isa[isa.index('amdhsa.kernels:'):]
    blocks = [b for b in meta.split('\n  - ') if re.search(r'\.name:\s+_Z\d+k_resize_', b)]
    assert len(blocks) == 2
    for b in blocks:
        for field in ('vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size'):
            assert int(re.search(r'\.%s:\s+(\d+)' % field, b).group(1)) == 0, field
    frames = code[code.index('k_resize_frames'):code.index('.Lfunc_end0')]
    assert 'global_load_dwordx4' in frames and 'ds_write_b128' in frames          # the 16-byte staging path
    assert 'flat_load' not in code and 'scratch_' not in code and 'atomic' not in code


def _table(rows):
    return (ctypes.c_longlong * (4 * len(rows)))(*[int(v) for r in rows for v in r])


def test_bad_arguments_are_refused_before_any_launch():
    """Every refusal happens on the host from the host copy of the table: no device is needed (or touched) to get FRTM_ERR_ARG."""
    from frtm_vos_amd import _hip
    L = _hip.lib()
    buf = (ctypes.c_ubyte * 4096)()
    p = ctypes.addressof(buf)                                     # stands in for the device pointers: nothing dereferences them
    ok = [(0, 10, 20, 0)]

    def frames(rows, n=None, planes=3, H=30, W=51, nbytes=4096, src=p, out=p, host=True, dev=p):
        t = _table(rows)
        return L.frtm_resize_frames_u8(src, nbytes, ctypes.addressof(t) if host else None, dev, len(rows) if n is None else n, planes, out, H, W, None)

    def labels(rows, n=None, H=30, W=51, nbytes=4096, src=p, out=p):
        t = _table(rows)
        return L.frtm_resize_labels_u8(src, nbytes, ctypes.addressof(t), p, len(rows) if n is None else n, out, H, W, None)
    for rows in ([(0, 0, 20, 0)], [(0, 10, 0, 0)], [(0, -3, 20, 0)], [(0, 10, 20, 2)], [(0, 10, 20, -1)], [(0, 20000, 1, 0)],
                 [(-1, 10, 20, 0)], [(4096 - 599, 10, 20, 0)], [(0, 10, 20, 0), (600, 10, 0, 0)]):
        assert frames(rows) == FRTM_ERR_ARG, rows
        assert b'frtm_resize_frames_u8' in L.frtm_last_error()
    for kw in (dict(H=0), dict(W=0), dict(H=-1), dict(W=20000), dict(n=0), dict(planes=0), dict(src=None), dict(out=None), dict(host=False),
               dict(dev=None), dict(nbytes=599), dict(planes=70000)):
        assert frames(ok, **kw) == FRTM_ERR_ARG, kw
    for rows in ([(0, 0, 20, 2)], [(0, 10, 0, 2)], [(0, 10, 20, 256)], [(0, 10, 20, -1)], [(4096 - 199, 10, 20, 2)]):
        assert labels(rows) == FRTM_ERR_ARG, rows
        assert b'frtm_resize_labels_u8' in L.frtm_last_error()
    for kw in (dict(H=0), dict(W=0), dict(n=0), dict(src=None), dict(out=None), dict(nbytes=199)):
        assert labels([(0, 10, 20, 2)], **kw) == FRTM_ERR_ARG, kw


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from frtm_vos_amd import ops
    table = torch.tensor([[0, 10, 20, 0]])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.resize_frames_u8(torch.zeros(600, dtype=torch.uint8), table, 3, (30, 51))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.resize_labels_u8(torch.zeros(200, dtype=torch.uint8), table, (30, 51))


# ---- the restatements ----
SIZES = [(45, 30), (77, 51), (83, 51), (51, 51), (219, 30), (102, 51), (33, 30), (40, 51), (20, 30), (30, 51), (1, 7), (7, 1), (1280, 854), (360, 480)]


@pytest.mark.parametrize('src,dst', SIZES)
def test_matrices_are_normalised(src, dst):
    for m in (R.area_matrix(src, dst), R.cubic_matrix(src, dst)):
        assert m.shape == (dst, src) and float(np.abs(m.sum(1) - 1).max()) < 1e-12
    a = R.area_matrix(src, dst)
    assert float(a.min()) >= 0
    if src == dst:
        assert np.array_equal(a, np.eye(src))
    if src >= dst:                                                # column sums: every source pixel is used exactly once overall
        assert float(np.abs(a.sum(0) * src / dst - 1).max()) < 1e-12


@pytest.mark.parametrize('src,dst', SIZES)
def test_restatements_agree_with_torch(src, dst):
    x = torch.from_numpy(np.random.default_rng(src * 1000 + dst).uniform(0, 255, (1, 1, 5, src)))
    want = F.interpolate(x, (5, dst), mode='bicubic', align_corners=False)[0, 0].numpy()          # (height unchanged: the identity there)
    assert float(np.abs(x[0, 0].numpy() @ R.cubic_matrix(src, dst).T - want).max()) < 1e-9
    if src < dst:
        want = F.interpolate(x, (5, dst), mode='bilinear', align_corners=False)[0, 0].numpy()
        assert float(np.abs(x[0, 0].numpy() @ R.area_matrix(src, dst).T - want).max()) < 1e-9
    if src % dst == 0:
        want = F.avg_pool2d(x, (1, src // dst))[0, 0].numpy()
        assert float(np.abs(x[0, 0].numpy() @ R.area_matrix(src, dst).T - want).max()) < 1e-9
    ids = torch.arange(src, dtype=torch.float32).view(1, 1, 1, src)
    assert np.array_equal(F.interpolate(ids, (1, dst), mode='nearest')[0, 0, 0].numpy().astype(np.int64), R.nearest_index(src, dst))


def test_area_means_by_hand():
    """3 -> 2: intervals [0, 1.5) and [1.5, 3): weights (1, 1/2) / 1.5 and (1/2, 1) / 1.5."""
    assert np.allclose(R.area_matrix(3, 2), [[2 / 3, 1 / 3, 0], [0, 1 / 3, 2 / 3]], atol=1e-15)
    assert np.array_equal(R.area_matrix(4, 2), [[0.5, 0.5, 0, 0], [0, 0, 0.5, 0.5]])
    assert np.array_equal(R.round_u8(np.array([0.5, 1.5, 2.5, -3.0, 255.5, 300.0])), [0, 2, 2, 0, 255, 255])          # ties to even, clamped


def test_near_tie_band_stays_under_the_cap():
    """The GPU tests allow 1 LSB inside the near-tie band only; this keeps the band itself small for every frame of non-integer ratio
    (on the reference alone: nothing here depends on the kernels)."""
    for shapes, seed, capped in ((R.MIXED, 11, R.CAPPED_MIXED), (R.EXTRA, 12, R.CAPPED_EXTRA)):
        frames = R.seeded_frames(shapes, seed)
        for k in capped:
            share = float(R.near_tie(R.resize_ref(frames[k], R.TARGET, shapes[k][2])).mean())
            print(shapes[k], 'share of outputs in the band %.4f' % share)
            assert share < R.BAND_CAP, (shapes[k], share)
