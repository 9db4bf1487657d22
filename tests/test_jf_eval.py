"""CPU tests of the GPU J / F evaluation (csrc/jf_eval.hip, ops.jf_counts, lib/davis.py, lib/evaluation.py): the ABI, the compiled form
of the kernels, the one place that turns integer counts into J and F, and the numpy path, which must keep giving what it gave."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
KERNELS = ['k_jf_planes', 'k_jf_match']


def test_jf_symbols_declared_exported_and_bound():
    from frtm_vos_amd import _hip
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read(), flags=re.S)
    L = _hip.lib()
    for name in ('frtm_jf_counts', 'frtm_jf_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert hasattr(L, name), name
        assert name in _hip.SIGNATURES, name
    # two bit planes per (frame, object), ceil(W / 64) 8-byte words per row
    assert L.frtm_jf_workspace_bytes(20, 480, 854, 2) == 20 * 2 * 2 * 480 * 14 * 8
    assert L.frtm_jf_workspace_bytes(1, 1, 1, 1) == 16 and L.frtm_jf_workspace_bytes(1, 1, 64, 1) == 16 and L.frtm_jf_workspace_bytes(1, 1, 65, 1) == 32


def test_jf_counts_refuses_bad_arguments_with_an_error_text():
    """Argument checks come before any device work, so they can be exercised without a GPU (the pointers are never followed)."""
    import ctypes
    from frtm_vos_amd import _hip
    L = _hip.lib()
    ids = (ctypes.c_int * 1)(1)
    ok = dict(pred=64, truth=64, label_bytes=1, T=1, H=4, W=4, ids=ids, K=1, r=8, counts=64, ws=64, ws_bytes=1 << 20, stream=None)
    for change, text in ((dict(r=0), b'radius'), (dict(r=65), b'radius'), (dict(label_bytes=2), b'label_bytes'), (dict(T=0), b'>= 1'), (dict(W=0), b'>= 1'),
                         (dict(H=65536, W=32768), b'2^31'), (dict(ws_bytes=8), b'workspace'), (dict(pred=None), b'null'), (dict(T=40000), b'split')):
        a = dict(ok, **change)
        rc = L.frtm_jf_counts(a['pred'], a['truth'], a['label_bytes'], a['T'], a['H'], a['W'], a['ids'], a['K'], a['r'], a['counts'], a['ws'], a['ws_bytes'],
                              a['stream'])
        assert rc == -1, change
        assert text in L.frtm_last_error(), (change, L.frtm_last_error())


@pytest.fixture(scope='module')
def jf_isa():
    assert os.path.exists(HIPCC), 'hipcc is needed to inspect the compiled kernels'
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'jf_eval.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'jf_eval.hip')], check=True, capture_output=True, cwd=d)
        return open(out).read()


@pytest.mark.parametrize('kernel', KERNELS)
def test_jf_kernels_spill_nothing(jf_isa, kernel):
    meta = jf_isa[jf_isa.index('amdhsa.kernels:'):]
    blocks = [b for b in meta.split('\n  - ') if re.search(r'\.name:\s+_Z%d%s[A-Z]' % (len(kernel), kernel), b)]
    assert len(blocks) == (2 if kernel == 'k_jf_planes' else 1), kernel              # uint8 and int32 label maps
    for b in blocks:
        assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', b).group(1)) == 0
        assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', b).group(1)) == 0
        assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', b).group(1)) == 0


def test_jf_kernels_count_with_popcount_and_integer_atomics_only(jf_isa):
    """Exactness is structural: every sum is an integer sum (population counts, integer atomics); no float atomic of any kind."""
    code = jf_isa[:jf_isa.index('amdhsa.kernels:')]
    assert 'bcnt' in code
    assert not re.search(r'global_atomic_\w*f32|global_atomic_\w*f64|buffer_atomic\w*(f32|f64|fadd|fmin|fmax)|ds_add_f32|ds_add_rtn_f32|ds_add_f64', code)
    assert not re.search(r'atomic\w*_(f16|bf16|pk_)', code)
    assert 'scratch_' not in code
    assert re.search(r'global_atomic_add(_u32)?\b', code)


def _masks(kind, rng, H=37, W=70):
    z = np.zeros((H, W), bool)
    a, b = z.copy(), z.copy()
    if kind == 'empty_prediction':
        b[5:20, 8:40] = True
    elif kind == 'empty_truth':
        a[5:20, 8:40] = True
    elif kind == 'disjoint':
        a[2:10, 2:12] = True
        b[25:35, 50:68] = True
    elif kind == 'identical':
        a[5:20, 8:40] = True
        b = a.copy()
    elif kind == 'overlap':
        a[5:20, 8:40] = True
        b[8:24, 10:45] = True
    elif kind == 'noise':
        a, b = rng.rand(H, W) < 0.3, rng.rand(H, W) < 0.3
    elif kind == 'full':
        a[:], b[:] = True, True
    else:
        assert kind == 'both_empty'
    return a, b


@pytest.mark.parametrize('kind', ['empty_prediction', 'empty_truth', 'both_empty', 'disjoint', 'identical', 'overlap', 'noise', 'full'])
def test_count_to_measure_functions_reproduce_the_mask_functions(kind):
    from frtm_vos_amd.lib import davis as D
    fg, gt = _masks(kind, np.random.RandomState(3))
    inter, union = int((fg & gt).sum()), int((fg | gt).sum())
    assert D.iou_from_counts(inter, union) == D.db_eval_iou(gt, fg) == D.davis_jaccard_measure(fg, gt)
    for bound_th in (0.008, 0.05, 1, 3):
        r = D.boundary_radius(fg.shape, bound_th)
        assert r == max(int(bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm(fg.shape))), 1)
        fb, gb = D.seg2bmap(fg), D.seg2bmap(gt)
        disk = D._disk(r)
        from scipy import ndimage
        fm = int((fb & ndimage.binary_dilation(gb, disk)).sum())
        gm = int((gb & ndimage.binary_dilation(fb, disk)).sum())
        got = D.f_from_counts(int(fb.sum()), int(gb.sum()), fm, gm)
        assert got == D.db_eval_boundary(fg, gt, bound_th), (kind, bound_th)
        if fb.any() and gb.any():
            assert D.boundary_counts(fg, gt, r) == (int(fb.sum()), int(gb.sum()), fm, gm)
    if kind == 'both_empty':
        assert D.iou_from_counts(0, 0) == 1.0 and D.f_from_counts(0, 0, 0, 0) == 1.0
    if kind == 'disjoint':
        assert D.iou_from_counts(inter, union) == 0.0 and D.db_eval_boundary(fg, gt) == 0.0
    if kind == 'identical':
        assert D.db_eval_boundary(fg, gt) == 1.0
    assert D.boundary_radius((480, 854)) == 8 and D.boundary_radius((1080, 1920)) == 18 and D.boundary_radius((3, 3)) == 1


def _sequence():
    """Six 40 x 60 frames, two moving rectangles; predictions = ground truth shifted and salted."""
    rng = np.random.RandomState(11)
    gts, prs = [], []
    for t in range(6):
        gt = np.zeros((40, 60), np.uint8)
        gt[5 + t:20 + t, 5:25] = 1
        gt[22:38, 30 + t:55] = 2
        pr = np.roll(gt, (1, -2), (0, 1))
        pr[rng.rand(40, 60) < 0.01] = 0
        gts.append(gt)
        prs.append(pr)
    return prs, gts


# values of the numpy path before the count functions were factored out (float repr round-trips exactly)
PINNED_J_AND_F = (64.21058628281759, 72.47987048721562, 55.94130207841954)
PINNED_RESULTS_MEAN = {'J': 0.7247987048721563, 'F': 0.5594130207841954}
PINNED_STATS_OBJ1_F = (0.5591436478921413, 1.0, 0.015724331793441126)


@pytest.mark.parametrize('form', ['numpy', 'cpu_tensor'])
def test_numpy_path_values_unchanged(form):
    from frtm_vos_amd.lib import evaluation as E
    prs, gts = _sequence()
    if form == 'cpu_tensor':
        prs, gts = [torch.from_numpy(p) for p in prs], [torch.from_numpy(g) for g in gts]
    assert E.j_and_f(prs, gts, [1, 2]) == PINNED_J_AND_F
    for m in 'JF':
        out = E.evaluate_results([('s', prs, gts, [1, 2])], m)
        assert out['mean'] == PINNED_RESULTS_MEAN[m]
        assert E.evaluate_dataset([('s', prs, gts, [1, 2])], m)['mean'] == PINNED_RESULTS_MEAN[m]
    assert E.evaluate_results([('s', prs, gts, [1, 2])], 'F')['per_sequence']['s'][1] == PINNED_STATS_OBJ1_F


def test_numpy_path_still_takes_what_it_took():
    """Nothing is refused on the numpy path that was accepted before: bool masks, int64 labels, float masks in db_eval_*, label lists
    of python lists, radii beyond the kernels' 64 px."""
    from frtm_vos_amd.lib import davis as D
    from frtm_vos_amd.lib import evaluation as E
    prs, gts = _sequence()
    assert E.j_and_f([p.astype(np.int64) for p in prs], [g.astype(np.int64) for g in gts], [1, 2]) == PINNED_J_AND_F
    assert E.j_and_f([p.tolist() for p in prs], [g.tolist() for g in gts], [1, 2]) == PINNED_J_AND_F
    assert E.j_and_f(np.stack(prs), torch.from_numpy(np.stack(gts)), (1, 2)) == PINNED_J_AND_F
    a, b = prs[2] == 1, gts[2] == 1
    assert D.db_eval_boundary(a.astype(np.float32), b.astype(np.float32)) == D.db_eval_boundary(a, b)
    assert D.db_eval_iou(b.astype(np.float64), a.astype(np.float64)) == D.db_eval_iou(b, a)
    assert D.db_eval_boundary(a, b, bound_th=100) == 1.0                      # every boundary pixel within 100 px on a 40 x 60 frame
    assert E.evaluate_dataset([], 'J')['per_sequence'] == {}


def test_jf_counts_has_no_cpu_path():
    from frtm_vos_amd import ops
    lb = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.jf_counts(lb, lb, [1], 1)
    with pytest.raises(TypeError):
        ops.jf_counts(lb.numpy(), lb.numpy(), [1], 1)


def test_evaluate_dataset_signature_keeps_its_defaults():
    import inspect
    from frtm_vos_amd.lib.evaluation import evaluate_dataset
    p = inspect.signature(evaluate_dataset).parameters
    assert list(p) == ['dset', 'results_path', 'measure', 'to_file', 'device'] and p['device'].default is None and p['to_file'].default is True
