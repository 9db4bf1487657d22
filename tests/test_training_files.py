"""CPU tests of the file-backed training sample sets (lib/training_datasets.py: DAVISDataset, YouTubeVOSDataset, raw_collate,
DeviceFrameResizer's mode rule), of the Trainer's collate / batch-transform hooks and of train.py's dataset options, on the tiny
trees of tests/_file_trees.py."""
import json

import numpy as np
import pytest
import torch

import _file_trees as trees


@pytest.fixture(scope='module')
def davis_root(tmp_path_factory):
    return trees.make_davis(tmp_path_factory.mktemp('davis'))


@pytest.fixture(scope='module')
def ytvos_root(tmp_path_factory):
    return trees.make_ytvos(tmp_path_factory.mktemp('ytvos'))


def _davis(root, tmp_path, **kw):
    from frtm_vos_amd.lib.training_datasets import DAVISDataset
    kw.setdefault('meta_file', tmp_path / 'davis_meta.pth')
    return DAVISDataset(root, **kw)


def _ytvos(root, tmp_path, **kw):
    from frtm_vos_amd.lib.training_datasets import YouTubeVOSDataset
    kw.setdefault('meta_file', tmp_path / 'ytvos_meta.pth')
    kw.setdefault('epoch_samples', 0)
    return YouTubeVOSDataset(root, **kw)


def _specs(d):
    return [s.encoded() for s in d.specs]


# ---- occlusion tables ----
def test_occlusions_equal_the_hand_computed_tables(davis_root, ytvos_root, tmp_path):
    d, y = _davis(davis_root, tmp_path), _ytvos(ytvos_root, tmp_path)
    assert np.array_equal(d.occlusions['alpha'], trees.DAVIS_OCC_A) and np.array_equal(d.occlusions['beta'], trees.OCC_B)
    assert np.array_equal(y.occlusions['0a1b2c'], trees.YTVOS_OCC_A) and np.array_equal(y.occlusions['3d4e5f'], trees.OCC_B)
    assert d.frame_names['alpha'] == ['%05d' % k for k in range(6)] and y.frame_names['3d4e5f'] == ['%05d' % (5 * k) for k in range(5)]
    # (sequence, object) pairs: the absent id 2 and the 3-frame sequences are out
    assert sorted(d.visible) == [('alpha', 1), ('alpha', 3), ('beta', 1)] and sorted(y.visible) == [('0a1b2c', 1), ('0a1b2c', 3), ('3d4e5f', 1)]
    assert d.visible[('alpha', 1)] == [0, 1, 3, 4, 5] and d.visible[('alpha', 3)] == [0, 2, 3, 4, 5] and y.visible[('0a1b2c', 3)] == list(range(6))
    assert len(d) == 3 and len(_davis(davis_root, tmp_path, epoch_repeats=4)) == 12 and len(_ytvos(ytvos_root, tmp_path, epoch_samples=2)) == 2
    with pytest.raises(ValueError, match='sample_size'):
        _davis(davis_root, tmp_path, sample_size=1)


def test_sampling_respects_visibility_and_is_a_function_of_seed_and_epoch(davis_root, tmp_path):
    from frtm_vos_amd.model.training_model import SampleSpec
    d = _davis(davis_root, tmp_path, epoch_repeats=5, seed=4)
    first = _specs(d)
    firsts = set()
    for epoch in range(12):
        d.set_epoch(epoch)
        for spec in d.specs:
            assert spec.obj_id != 2 and spec.seq_name in ('alpha', 'beta')
            assert not d.occlusions[spec.seq_name][spec.frames[0], spec.obj_id]                    # frame 0 shows the object
            assert spec.frame0_id == spec.frames[0] and len(spec.frames) == 3 and len(set(spec.frames)) == 3
            assert all(0 <= t < d.n_frames[spec.seq_name] for t in spec.frames)
            assert SampleSpec.from_encoded([spec.encoded()])[0].encoded() == spec.encoded()
            firsts.add((spec.seq_name, spec.obj_id, spec.frames[0]))
    assert ('alpha', 1, 2) not in firsts and ('alpha', 3, 1) not in firsts
    assert {f for s, o, f in firsts if (s, o) == ('alpha', 1)} == {0, 1, 3, 4, 5}                 # 60 draws over 5 frames: all of them turn up
    d.set_epoch(1)
    second = _specs(d)
    d.set_epoch(0)
    assert _specs(d) == first and second != first
    assert _specs(_davis(davis_root, tmp_path, epoch_repeats=5, seed=4)) == first                 # a fresh instance draws the same
    assert _specs(_davis(davis_root, tmp_path, epoch_repeats=5, seed=5)) != first


# ---- the metadata file ----
def test_meta_file_round_trips_in_the_reference_layout(davis_root, tmp_path, monkeypatch):
    from frtm_vos_amd.lib.training_datasets import DAVISDataset, default_meta_file
    file = tmp_path / 'sub' / 'davis_meta.pth'
    d = _davis(davis_root, tmp_path, meta_file=file)
    assert [p.name for p in file.parent.iterdir()] == ['davis_meta.pth']                          # written atomically, no temporary left
    meta = torch.load(file, weights_only=False)
    assert set(meta) == {'frame_names', 'occlusions'} and set(meta['occlusions']) == set(meta['frame_names']) == {'alpha', 'beta', 'gamma'}
    for seq, occ in meta['occlusions'].items():
        assert isinstance(occ, np.ndarray) and occ.dtype == np.bool_ and occ.ndim == 2 and occ.shape[0] == len(meta['frame_names'][seq])
        assert isinstance(meta['frame_names'][seq], list) and all(isinstance(s, str) for s in meta['frame_names'][seq])
    assert meta['occlusions']['alpha'].shape == (6, 4) and meta['occlusions']['beta'].shape == (5, 2) and meta['occlusions']['gamma'].shape == (3, 2)
    monkeypatch.setattr(DAVISDataset, 'pixel_counts', lambda *a: pytest.fail('the stored table was not used'))
    again = _davis(davis_root, tmp_path, meta_file=file)
    assert _specs(again) == _specs(d) and np.array_equal(again.occlusions['alpha'], trees.DAVIS_OCC_A)
    # a table from elsewhere (the reference's file) is used exactly as it is
    theirs = dict(frame_names=meta['frame_names'], occlusions=dict(meta['occlusions']))
    theirs['occlusions']['alpha'] = np.ones((6, 4), dtype=bool)
    theirs['occlusions']['alpha'][4, 1] = False
    torch.save(theirs, tmp_path / 'theirs.pth')
    t = _davis(davis_root, tmp_path, meta_file=tmp_path / 'theirs.pth', epoch_repeats=6)
    assert sorted(t.visible) == [('alpha', 1), ('beta', 1)] and all(s.frames[0] == 4 for s in t.specs if s.seq_name == 'alpha')
    assert default_meta_file('davis', tmp_path / 'ws') == tmp_path / 'ws' / 'meta' / 'davis_meta.pth'


@pytest.mark.parametrize('override,flipped', [
    ({'threshold': 0.2}, [(1, 3)]),                      # 140 / 600 = 0.233 passes a 0.2 threshold; 90 px stays under the hard minimum
    ({'never_occluded': True}, [(1, 3)]),
    ({'visible': [[1, 2, 3]]}, [(1, 3)]),
    ({'visible': [[0, None, None]]}, [(1, 3)]),
    ({'visible': [[2, 3, 1]]}, []),                      # frame 2 of object 1 passes the fraction rule but not the hard minimum
    ({'threshold': 0.31}, [(4, 1)]),                     # 120 / 400 = 0.3 now falls below
])
def test_overrides_change_exactly_the_flags_they_name(davis_root, tmp_path, override, flipped):
    want = trees.DAVIS_OCC_A.copy()
    for f, o in flipped:
        want[f, o] = not want[f, o]
    d = _davis(davis_root, tmp_path, overrides={'alpha': override})
    assert np.array_equal(d.occlusions['alpha'], want) and np.array_equal(d.occlusions['beta'], trees.OCC_B)
    (tmp_path / 'o.json').write_text(json.dumps({'alpha': override}))
    j = _davis(davis_root, tmp_path, overrides=tmp_path / 'o.json', meta_file=tmp_path / 'from_json.pth')
    assert np.array_equal(j.occlusions['alpha'], want)
    with pytest.raises(ValueError, match='overrides'):
        _davis(davis_root, tmp_path, overrides={'alpha': {'treshold': 0.2}}, meta_file=tmp_path / 'typo.pth')


# ---- samples and collation ----
def test_samples_keep_native_sizes_through_raw_collate(ytvos_root, tmp_path):
    from frtm_vos_amd.lib.training_datasets import raw_collate
    from frtm_vos_amd.model.training_model import SampleSpec
    y = _ytvos(ytvos_root, tmp_path)
    images, labels, meta = y[0]
    assert len(images) == len(labels) == 3 and isinstance(meta, str)
    loader = torch.utils.data.DataLoader(y, batch_size=3, collate_fn=raw_collate)
    images, labels, meta = next(iter(loader))
    specs = SampleSpec.from_encoded(meta)
    assert len(images) == len(labels) == 3 and all(len(f) == 3 for f in images + labels) and len(meta) == 3
    assert {s.seq_name for s in specs} == {'0a1b2c', '3d4e5f'}                                    # both sizes in one batch
    for t in range(3):
        for b, spec in enumerate(specs):
            h, w = trees.YTVOS_SIZES[spec.seq_name]
            assert images[t][b].dtype == torch.uint8 and tuple(images[t][b].shape) == (3, h, w)
            assert labels[t][b].dtype == torch.uint8 and tuple(labels[t][b].shape) == (1, h, w)
            areas = trees.A_AREAS if spec.seq_name == '0a1b2c' else trees.B_AREAS                  # raw ids, not yet relabelled
            for obj, a in areas.items():
                assert int((labels[t][b] == obj).sum()) == a[spec.frames[t]]
            assert torch.equal(images[t][b], y[b][0][t])


def test_resizer_mode_rule(davis_root, ytvos_root, tmp_path):
    from frtm_vos_amd.lib.training_datasets import DeviceFrameResizer
    d, y = _davis(davis_root, tmp_path), _ytvos(ytvos_root, tmp_path)
    r = DeviceFrameResizer((480, 854), 'cuda:0', datasets=[d, y])
    assert r.mode('alpha', 480) == 'area' and r.mode('alpha', 360) == 'area'                       # DAVIS: always
    assert r.mode('0a1b2c', 720) == 'area' and r.mode('0a1b2c', 481) == 'area'                     # 480 / h < 1
    assert r.mode('0a1b2c', 480) == 'cubic' and r.mode('3d4e5f', 360) == 'cubic'


# ---- driver ----
class _Recorder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(2))
        self.seen = []

    def forward(self, images, labels, meta):
        self.seen.append((images, labels, meta))
        loss = (self.w ** 2).sum()
        loss.backward()
        return {'stats/loss': float(loss.detach()), 'stats/accuracy': 0.5, 'stats/fcache_hits': len(meta)}


def _trainer(tmp_path, dataset, **kw):
    from frtm_vos_amd.lib.training import Trainer
    model = _Recorder()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    return Trainer('run', model, opt, sched, dataset, tmp_path / 'ckpt', tmp_path / 'log', max_epochs=1, batch_size=2, **kw), model


def test_trainer_hands_the_model_what_the_transform_returned(ytvos_root, tmp_path):
    from frtm_vos_amd.lib.training_datasets import raw_collate
    y = _ytvos(ytvos_root, tmp_path)
    got = []

    def transform(batch):
        images, labels, meta = batch
        got.append(batch)
        assert isinstance(images[0], list) and images[0][0].dim() == 3                             # raw_collate's form arrives here
        return ['images', len(got)], ['labels', len(got)], list(meta)
    tr, model = _trainer(tmp_path, y, collate_fn=raw_collate, batch_transform=transform)
    tr.train()
    assert len(got) == 2 and len(model.seen) == 2                                                  # 3 samples, batches of 2
    for k, (images, labels, meta) in enumerate(model.seen, 1):
        assert images == ['images', k] and labels == ['labels', k] and meta == got[k - 1][2]
    assert sorted(m for b in got for m in b[2]) == sorted(_specs(y))


def test_trainer_without_hooks_collates_as_before(tmp_path):
    from frtm_vos_amd.lib.training_datasets import SyntheticTrainingDataset
    d = SyntheticTrainingDataset(n_sequences=4, n_frames=6, size=(96, 128), seed=3)
    tr, model = _trainer(tmp_path, d)
    assert tr.collate_fn is None and tr.batch_transform is None
    tr.train()
    assert len(d) == 4 and len(model.seen) == 2
    images, labels, meta = model.seen[0]
    assert len(images) == 3 and all(isinstance(i, torch.Tensor) and tuple(i.shape) == (2, 3, 96, 128) and i.dtype == torch.uint8 for i in images)
    assert all(tuple(l.shape) == (2, 1, 96, 128) for l in labels) and len(meta) == 2


def test_train_command_line_dataset_options(davis_root, ytvos_root, tmp_path):
    from frtm_vos_amd.train import file_datasets, parse_args
    a = parse_args(['x', '--dset', 'davis', '--davis-path', str(davis_root)])
    assert a.dset == 'davis' and a.davis_path == str(davis_root) and a.ytvos_path is None and a.num_workers == 0
    assert a.ytvos_sequences_file is None and a.occlusion_overrides is None
    assert parse_args(['x']).dset == 'synthetic'
    (tmp_path / 'ids.txt').write_text('3d4e5f\n')
    (tmp_path / 'o.json').write_text(json.dumps({'alpha': {'threshold': 0.2}}))
    b = parse_args(['x', '--dset', 'davis+ytvos', '--davis-path', str(davis_root), '--ytvos-path', str(ytvos_root), '--num-workers', '2',
                    '--ytvos-sequences-file', str(tmp_path / 'ids.txt'), '--occlusion-overrides', str(tmp_path / 'o.json')])
    assert b.num_workers == 2
    dv, yt = file_datasets(b, tmp_path / 'ws')
    assert (dv.name, yt.name) == ('davis', 'ytvos2018') and yt.sequences == ['3d4e5f'] and not dv.occlusions['alpha'][1, 3]
    assert len(dv) == 3 * 8 and len(yt) == 1                                                       # the reference's epoch sizes
    assert sorted(p.name for p in (tmp_path / 'ws' / 'meta').iterdir()) == ['davis_meta.pth', 'ytvos2018_meta.pth']
    with pytest.raises(SystemExit):
        file_datasets(parse_args(['x', '--dset', 'ytvos']), tmp_path / 'ws')
    with pytest.raises(SystemExit):
        parse_args(['x', '--dset', 'coco'])
