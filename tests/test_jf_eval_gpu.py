"""GPU tests of the J / F evaluation kernels (csrc/jf_eval.hip) and of the evaluation functions on device label maps.  The measures are
integer counting problems, so every comparison between the GPU path and the numpy path is ``==``: the same six integers per
(frame, object), and from them, with the same float64 expressions, the same J and F bit for bit.  No case is sampled or left out."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES = [(1, 1), (1, 70), (2, 129), (5, 3), (33, 64), (64, 65), (60, 80), (97, 131), (480, 854), (1080, 1920)]
PROTOCOL = 0.008                      # bound_th of the DAVIS protocol: 8 px at 480p, 18 px at 1080p
EXPLICIT_RADII = [1, 2, 3, 40, 64]    # go in as bound_th >= 1, which both paths take as pixels
KINDS = ['blobs', 'borders', 'salt2', 'salt50', 'empty_prediction', 'empty_truth', 'both_empty', 'full']


def _numpy_counts(pred, truth, ids, bound_th):
    """(T,K,6) counts with the numpy definition of lib/davis.py."""
    from frtm_vos_amd.lib import davis as D
    T = len(pred)
    out = np.zeros((T, len(ids), 6), np.int64)
    r = D.boundary_radius(pred[0].shape, bound_th)
    for t in range(T):
        for k, oid in enumerate(ids):
            fg, gt = pred[t] == oid, truth[t] == oid
            out[t, k, 0], out[t, k, 1] = (fg & gt).sum(), (fg | gt).sum()
            fb, gb = D.seg2bmap(fg), D.seg2bmap(gt)
            out[t, k, 2], out[t, k, 3] = fb.sum(), gb.sum()
            if fb.any() and gb.any():
                out[t, k, 4], out[t, k, 5] = D._within(fb, gb, r).sum(), D._within(gb, fb, r).sum()
    return out


def _blob(H, W, cy, cx, ry, rx, wobble, phase):
    """Smooth star-shaped blob: an ellipse whose radius wobbles with the angle."""
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    dy, dx = (yy - cy) / max(ry, 0.5), (xx - cx) / max(rx, 0.5)
    ang = np.arctan2(dy, dx)
    return dy * dy + dx * dx <= (1 + wobble * np.sin(3 * ang + phase)) ** 2


def _frame(kind, H, W, rng):
    """(pred, truth) uint8 label maps with objects 1 and 2 (id 7 never occurs)."""
    pred, truth = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    if kind == 'blobs':
        truth[_blob(H, W, 0.4 * H, 0.35 * W, 0.22 * H, 0.2 * W, 0.2, 0.3)] = 1
        truth[_blob(H, W, 0.6 * H, 0.7 * W, 0.25 * H, 0.15 * W, 0.3, 1.1)] = 2
        pred[_blob(H, W, 0.4 * H + 2, 0.35 * W - 3, 0.2 * H, 0.22 * W, 0.2, 0.5)] = 1
        pred[_blob(H, W, 0.6 * H - 1, 0.7 * W + 2, 0.25 * H, 0.17 * W, 0.25, 1.0)] = 2
    elif kind == 'borders':           # object 1 covers the four corners, object 2 the middle of each border
        for m, s in ((truth, 0), (pred, 1)):
            for cy in (0, H - 1):
                for cx in (0, W - 1):
                    m[_blob(H, W, cy, cx, 0.2 * H + s, 0.15 * W + 2 * s, 0.2, 0.7)] = 1
            for cy, cx in ((0, W / 2), (H - 1, W / 2), (H / 2, 0), (H / 2, W - 1)):
                m[_blob(H, W, cy, cx + s, 0.12 * H + 1, 0.12 * W + 1, 0.1, 0.2)] = 2
    elif kind in ('salt2', 'salt50'):
        p = 0.02 if kind == 'salt2' else 0.5
        truth[_blob(H, W, 0.5 * H, 0.5 * W, 0.3 * H, 0.3 * W, 0.2, 0.0)] = 1
        pred[:] = truth
        for m in (pred, truth):
            salt = rng.rand(H, W) < p
            m[salt] = rng.randint(0, 3, size=(H, W))[salt]
    elif kind == 'empty_prediction':
        truth[_blob(H, W, 0.5 * H, 0.4 * W, 0.3 * H, 0.2 * W, 0.2, 0.0)] = 1
        truth[_blob(H, W, 0.5 * H, 0.8 * W, 0.2 * H, 0.1 * W, 0.1, 0.0)] = 2
    elif kind == 'empty_truth':
        pred[_blob(H, W, 0.5 * H, 0.4 * W, 0.3 * H, 0.2 * W, 0.2, 0.0)] = 1
        pred[_blob(H, W, 0.5 * H, 0.8 * W, 0.2 * H, 0.1 * W, 0.1, 0.0)] = 2
    elif kind == 'full':
        pred[:], truth[:] = 1, 1
        truth[H // 2:, :] = 2         # object 2: the lower half of the truth, nothing of the prediction
    else:
        assert kind == 'both_empty'
    return pred, truth


def _case(H, W, seed):
    rng = np.random.RandomState(seed)
    frames = [_frame(k, H, W, rng) for k in KINDS]
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])


def _check_counts(pred, truth, bound_th, what):
    """uint8 maps with ids (1, 2, 7) and the same maps as int32 with object 2 renamed 300: six integers == numpy, measures == numpy, three
    calls equal."""
    from frtm_vos_amd import ops
    from frtm_vos_amd.lib import davis as D
    ids = [1, 2, 7]
    want = _numpy_counts(pred, truth, ids, bound_th)
    r = D.boundary_radius(pred.shape[-2:], bound_th)
    pd, td = torch.from_numpy(pred).to(DEV), torch.from_numpy(truth).to(DEV)
    got = D.device_counts(pd, td, ids, bound_th)
    assert got.shape == want.shape and got.dtype == np.int64
    assert np.array_equal(got, want), (what, 'uint8', np.argwhere(got != want)[:8].tolist(), got[got != want][:8], want[got != want][:8])
    first = ops.jf_counts(pd, td, ids, r)
    assert first.dtype == torch.int32 and first.is_cuda and tuple(first.shape) == want.shape
    for _ in range(2):
        assert torch.equal(ops.jf_counts(pd, td, ids, r), first), what
    assert np.array_equal(first.cpu().numpy(), want)
    p32, t32 = pred.astype(np.int32), truth.astype(np.int32)
    p32[pred == 2], t32[truth == 2] = 300, 300
    assert np.array_equal(p32 == 300, pred == 2) and np.array_equal(t32 == 300, truth == 2)      # so `want` holds for ids (1, 300, 7) too
    got32 = D.device_counts(torch.from_numpy(p32).to(DEV), torch.from_numpy(t32).to(DEV), [1, 300, 7], bound_th)
    assert np.array_equal(got32, want), (what, 'int32')
    assert (want[:, 2] == 0).all()                                                                  # the id that is in neither map
    for t in range(len(pred)):
        for k, oid in enumerate(ids):
            fg, gt = pred[t] == oid, truth[t] == oid
            assert D.measure_from_counts(got[t, k], 'J') == D.davis_jaccard_measure(fg, gt)
            assert D.measure_from_counts(got[t, k], 'F') == D.davis_f_measure(fg, gt, bound_th)


@pytest.mark.parametrize('size', SIZES, ids=['%dx%d' % s for s in SIZES])
def test_counts_equal_numpy(size):
    """Every size with the protocol's radius and the explicit ones; 1080 x 1920 at r = 18 (the protocol's) and r = 64 only: its numpy side
    costs up to a second per map."""
    from frtm_vos_amd.lib import davis as D
    H, W = size
    pred, truth = _case(H, W, seed=H * 10007 + W)
    if size == (480, 854):
        assert D.boundary_radius(size, PROTOCOL) == 8
    if size == (1080, 1920):
        assert D.boundary_radius(size, PROTOCOL) == 18
    for bound_th in [PROTOCOL] + (EXPLICIT_RADII if size != (1080, 1920) else [64]):
        _check_counts(pred, truth, bound_th, (size, bound_th))


def test_counts_single_frame_and_frames_beyond_one_chunk():
    """T = 1, and a sequence long enough for ops.jf_counts to split it over frames (its workspace budget): the chunks join seamlessly."""
    from frtm_vos_amd import _hip, ops
    from frtm_vos_amd.lib import davis as D
    H, W, ids = 97, 131, [1, 2, 7]
    pred, truth = _case(H, W, seed=5)
    for t in (0, 3):
        got = D.device_counts(torch.from_numpy(pred[t:t + 1]).to(DEV), torch.from_numpy(truth[t:t + 1]).to(DEV), ids)
        assert np.array_equal(got, _numpy_counts(pred[t:t + 1], truth[t:t + 1], ids, PROTOCOL))
    per_frame = _hip.lib().frtm_jf_workspace_bytes(1, H, W, len(ids))
    step = min(ops.JF_WS_BUDGET // per_frame, 65535 // (2 * len(ids)))
    T = step + 98
    assert step >= 1 and T <= 2600
    rng = np.random.RandomState(17)
    truth = np.zeros((T, H, W), np.uint8)
    pred = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        y, x, h, w = rng.randint(0, H - 20), rng.randint(0, W - 30), rng.randint(5, 20), rng.randint(5, 30)
        truth[t, y:y + h, x:x + w] = 1
        truth[t, (y + 40) % H:(y + 40) % H + h // 2 + 1, x:x + w] = 2
        pred[t] = np.roll(truth[t], (rng.randint(-3, 4), rng.randint(-3, 4)), (0, 1))
        salt = rng.rand(H, W) < 0.003
        pred[t][salt] = rng.randint(0, 3, size=(H, W))[salt]
    got = D.device_counts(torch.from_numpy(pred).to(DEV), torch.from_numpy(truth).to(DEV), ids)
    want = _numpy_counts(pred, truth, ids, PROTOCOL)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    assert want[step - 1:step + 1, :2, 2:4].min() > 0                                     # both sides of the seam carry real counts


def test_counts_more_ids_than_one_launch_takes():
    """The first pass takes 16 ids per launch (four counters each in the 64 lanes of a wave): 21 ids in one call, in no particular order,
    one of them absent, uint8 and int32."""
    from frtm_vos_amd.lib import davis as D
    rng = np.random.RandomState(23)
    H, W, T = 64, 150, 3
    truth = np.zeros((T, H, W), np.uint8)
    for t in range(T):
        for oid in range(1, 21):
            y, x = rng.randint(0, H - 8), rng.randint(0, W - 12)
            truth[t, y:y + rng.randint(3, 16), x:x + rng.randint(3, 24)] = oid
    pred = np.roll(truth, (1, -2), (1, 2))
    salt = rng.rand(T, H, W) < 0.01
    pred[salt] = rng.randint(0, 21, size=pred.shape)[salt]
    ids = [int(v) for v in rng.permutation(20) + 1] + [99]
    want = _numpy_counts(pred, truth, ids, 3)
    assert (want[:, :20, 3] > 0).any(axis=0).all() and (want[:, 20] == 0).all()
    for dt in (np.uint8, np.int32):
        got = D.device_counts(torch.from_numpy(pred.astype(dt)).to(DEV), torch.from_numpy(truth.astype(dt)).to(DEV), ids, 3)
        assert np.array_equal(got, want), (dt, np.argwhere(got != want)[:8].tolist())


def test_g10_fixture_on_the_device(golden):
    """Fixture G10 (recorded from the reference's lib/davis.py): the gates tests/test_cpu_host.py holds the numpy path to, and exact
    equality with the numpy path."""
    from collections import OrderedDict as odict
    from frtm_vos_amd.lib import davis as D
    g = golden('g10_davis')
    for k in range(12):
        H, W = [int(v) for v in g['shape%d' % k]]
        a = np.unpackbits(g['a%d' % k])[:H * W].reshape(H, W).astype(bool)
        b = np.unpackbits(g['b%d' % k])[:H * W].reshape(H, W).astype(bool)
        bm = np.unpackbits(g['bmap%d' % k])[:H * W].reshape(H, W).astype(bool)
        # prediction = b, ground truth = a, as in davis_jaccard_measure(b, a) / davis_f_measure(b, a)
        c = D.device_counts(torch.from_numpy(b.astype(np.uint8))[None].to(DEV), torch.from_numpy(a.astype(np.uint8))[None].to(DEV), [1])[0, 0]
        assert c[3] == int(bm.sum()) == int(D.seg2bmap(a).sum()), k
        assert c[2] == int(D.seg2bmap(b).sum()), k
        xs, ys = np.minimum(np.arange(W) + 1, W - 1), np.minimum(np.arange(H) + 1, H - 1)
        assert np.array_equal((a != a[:, xs]) | (a != a[ys, :]) | (a != a[ys][:, xs]), bm), k      # the kernel's form of seg2bmap
        J, F = D.measure_from_counts(c, 'J'), D.measure_from_counts(c, 'F')
        assert abs(J - float(g['J'][k])) < 1e-6 and abs(F - float(g['F'][k])) < 1e-12, k
        assert J == D.davis_jaccard_measure(b, a) and F == D.davis_f_measure(b, a), k
    ann, seg, ann_d, seg_d = odict(), odict(), odict(), odict()
    for t in range(7):
        ann['%05d' % t] = torch.from_numpy(g['seq_ann%d' % t])[None]
        seg['%05d' % t] = torch.from_numpy(g['seq_seg%d' % t])[None]
        ann_d['%05d' % t], seg_d['%05d' % t] = ann['%05d' % t].to(DEV), seg['%05d' % t].to(DEV)
    info = {1: '00000', 2: '00002'}
    for measure in 'JF':
        r = D.evaluate_sequence(seg_d, ann_d, info, measure=measure)
        n = D.evaluate_sequence(seg, ann, info, measure=measure)
        raw, raw_n, ref = np.stack([r['raw'][1], r['raw'][2]]), np.stack([n['raw'][1], n['raw'][2]]), g['seq_%s_raw' % measure]
        assert np.array_equal(np.isnan(raw), np.isnan(ref)) and np.array_equal(np.isnan(raw), np.isnan(raw_n))
        assert np.allclose(np.nan_to_num(raw), np.nan_to_num(ref), rtol=0, atol=1e-6)
        assert np.array_equal(np.nan_to_num(raw), np.nan_to_num(raw_n))
        for st in ('mean', 'recall', 'decay', 'std'):
            assert np.allclose(r[st], g['seq_%s_%s' % (measure, st)], rtol=0, atol=1e-6), (measure, st)
            assert r[st] == n[st], (measure, st)


def test_synthetic_sequence_on_device_lists_equals_numpy():
    """The benchmark's shape: 480 x 854, 20 frames, 2 objects; predictions = ground truth under seeded shifts and noise."""
    from frtm_vos_amd.lib import evaluation as E
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    seq = SyntheticSequence('jfeval', 20, (480, 854), 2, seed=21)
    rng = np.random.RandomState(4)
    gt = [g.reshape(480, 854).numpy() for g in seq.gt]
    pred = []
    for t, g in enumerate(gt):
        p = np.roll(g, (int(rng.randint(-4, 5)), int(rng.randint(-4, 5))), (0, 1))
        salt = rng.rand(480, 854) < 0.002
        p[salt] = rng.randint(0, 3, size=p.shape)[salt]
        pred.append(np.ascontiguousarray(p))
    gt_d = [g.to(DEV) for g in seq.gt]                                              # (1,H,W) each, like the sequence holds them
    pred_d = [torch.from_numpy(p)[None].to(DEV) for p in pred]
    for m in 'JF':
        got, want = E.evaluate_sequence(pred_d, gt_d, seq.obj_ids, m), E.evaluate_sequence(pred, gt, seq.obj_ids, m)
        assert list(got) == list(want) == seq.obj_ids
        for oid in seq.obj_ids:
            assert len(got[oid]) == 18 and got[oid] == want[oid], (m, oid)
        assert 0.3 < np.mean(want[1]) < 1.0
    assert E.j_and_f(pred_d, gt_d, seq.obj_ids) == E.j_and_f(pred, gt, seq.obj_ids)
    stacked = (torch.stack(pred_d).reshape(20, 480, 854), torch.stack(gt_d).reshape(20, 480, 854))
    assert E.j_and_f(stacked[0], stacked[1], seq.obj_ids) == E.j_and_f(pred, gt, seq.obj_ids)            # one (T,H,W) tensor per side
    res = E.evaluate_results([('s', pred_d, gt_d, seq.obj_ids)], 'F')
    assert res == E.evaluate_results([('s', pred, gt, seq.obj_ids)], 'F')


def test_tracker_output_goes_into_j_and_f_as_it_is():
    from oracle import make_golden_jf as JF
    from test_north_star_gpu import _hip_tracker
    from frtm_vos_amd.lib import evaluation as E
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    torch.set_grad_enabled(False)
    size = (480, 854)
    seq = SyntheticSequence('jftrk', 6, size, 2, seed=33)
    trk = _hip_tracker('resnet18', JF.refiner_for('resnet18'), fast=True)
    labels, _ = trk.run_sequence(seq)
    assert len(labels) == 6 and all(l.is_cuda for l in labels)
    gt_d = [g.to(DEV) for g in seq.gt]
    got = E.j_and_f(labels, gt_d, seq.obj_ids)
    want = E.j_and_f([l.reshape(size).cpu().numpy() for l in labels], [g.reshape(size).numpy() for g in seq.gt], seq.obj_ids)
    assert got == want
    assert all(np.isfinite(v) for v in got)


def _tiny_davis(tmp_path):
    """The tree of tests/test_cpu_host.py: test_evaluate_dataset_reference_signature."""
    from PIL import Image
    from frtm_vos_amd.lib.datasets import DAVISDataset
    from frtm_vos_amd.lib.image import imwrite_indexed
    root, res = tmp_path / 'DAVIS', tmp_path / 'results'
    (root / 'ImageSets' / '2017').mkdir(parents=True)
    (root / 'ImageSets' / '2017' / 'val.txt').write_text('cows\n')
    (root / 'JPEGImages' / '480p' / 'cows').mkdir(parents=True)
    (root / 'Annotations' / '480p' / 'cows').mkdir(parents=True)
    (res / 'cows').mkdir(parents=True)
    for t in range(6):
        Image.fromarray(np.zeros((40, 60, 3), np.uint8)).save(root / 'JPEGImages' / '480p' / 'cows' / ('%05d.jpg' % t))
        gt = torch.zeros(40, 60, dtype=torch.uint8)
        gt[5 + t:20 + t, 5:25] = 1
        gt[22:38, 30 + t:55] = 2
        pr = gt.clone()
        pr[5 + t:8 + t, 5:25] = 0                                  # object 1 loses 3 of 15 rows -> J = 0.8
        imwrite_indexed(root / 'Annotations' / '480p' / 'cows' / ('%05d.png' % t), gt)
        imwrite_indexed(res / 'cows' / ('%05d.png' % t), pr)
    return DAVISDataset(root, '2017', 'val', all_annotations=True), res


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])
    if isinstance(a, float) and np.isnan(a):
        return isinstance(b, float) and np.isnan(b)
    return a == b


def test_evaluate_dataset_on_the_device_writes_the_same_file(tmp_path, capsys):
    from frtm_vos_amd.lib.evaluation import evaluate_dataset
    dset, res = _tiny_davis(tmp_path)
    for m in 'JF':
        host = evaluate_dataset(dset, res, m, device=None)
        text_host = (res / ('evaluation-%s.txt' % m)).read_bytes()
        printed_host = capsys.readouterr().out
        (res / ('evaluation-%s.txt' % m)).unlink()
        dev = evaluate_dataset(dset, res, m, device=DEV)
        assert (res / ('evaluation-%s.txt' % m)).read_bytes() == text_host and len(text_host) > 50
        assert capsys.readouterr().out == printed_host
        assert _same(dev, host), m
    assert abs(evaluate_dataset(dset, res, 'J', device='cuda')['mean'] - 0.9) < 1e-6


def test_refusals_on_the_device_path():
    from frtm_vos_amd import ops
    from frtm_vos_amd.lib import davis as D
    from frtm_vos_amd.lib import evaluation as E
    lb = torch.zeros(3, 16, 16, dtype=torch.uint8)
    lb[:, 4:9, 4:9] = 1
    d = lb.to(DEV)
    with pytest.raises(ValueError, match='numpy'):
        D.device_counts(d, d, [1], bound_th=65)
    with pytest.raises(ValueError):
        ops.jf_counts(d, d, [1], 65)
    with pytest.raises(ValueError):
        ops.jf_counts(d, d, [1], 0)
    assert np.array_equal(D.device_counts(d, d, [1], bound_th=64), _numpy_counts(lb.numpy(), lb.numpy(), [1], 64))       # 64 itself is served
    for call in (lambda: E.j_and_f(d, lb, [1]), lambda: E.evaluate_sequence(list(d), list(lb), [1], 'F'),
                 lambda: E.evaluate_sequence([d[0], lb[1], d[2]], list(d), [1], 'J')):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        E.j_and_f(d.float(), d.float(), [1])
    with pytest.raises(ValueError):
        E.j_and_f(d, d[:, :8], [1])
    with pytest.raises(ValueError):
        E.j_and_f(list(d), list(d[:2]) + [d[2, :8]], [1])
    # 8000-px diagonals are where the protocol's radius passes 64: refused on the device, by name of the way out
    big = torch.zeros(1, 1, 8200, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match='numpy'):
        D.device_counts(big, big, [1])
