"""Sample sets for refiner training (counterpart of the reference's lib/training_datasets.py, written against its interface).

The contract a training dataset fulfils, and ``TrainerModel.forward`` consumes after the DataLoader's default collate:

    dataset[i] -> (images, labels, meta)
        images   ``sample_size`` uint8 tensors (3,H,W): frames of ONE sequence; frame 0 is one in which the object is visible (the target
                 model is fitted on it), the others are drawn from the rest of the sequence without replacement
        labels   ``sample_size`` uint8 tensors (1,H,W): the chosen object relabelled to 1, everything else 0
        meta     ``SampleSpec(seq_name, obj_id, frames, frame0_id).encoded()``: the identity under which the target model is cached

    len(dataset)            samples per epoch: (sequence, object) pairs (``epoch_samples`` of them drawn at random if > 0) times ``epoch_repeats``
    dataset.set_epoch(e)    redraws the samples from a generator seeded by (seed, e): a resumed run draws what an uninterrupted one would

``SyntheticTrainingDataset`` is the implementation that needs no files.

``DAVISDataset`` / ``YouTubeVOSDataset`` (``FileTrainingDataset``) read the datasets from disk with the reference's constructor arguments.
They differ from the contract above in ONE point: ``dataset[i]`` returns the decoded frames at their NATIVE size -- uint8 (3,h,w) images
and (1,h,w) maps of raw label ids -- because frames of one batch differ in size (YouTube-VOS) and the resize to the training size is
device work.  ``raw_collate`` keeps such samples as lists, ``DeviceFrameResizer`` packs a batch, copies it to the device once and
resamples every frame and label in one launch each (csrc/frame_resize.hip) into exactly what ``TrainerModel.forward`` takes:

    Trainer(..., dataset, collate_fn=raw_collate, batch_transform=DeviceFrameResizer((480, 854), device, datasets=[dataset]))

Which first frames are eligible comes from a per-sequence occlusion table, computed once from the annotations and stored in the
reference's ``<name>_meta.pth`` layout (``FileTrainingDataset.load_meta``)."""
import json
import os
from pathlib import Path

import numpy as np
import torch

from .._hip import normalize_device
from ..model.training_model import SampleSpec
from .synthetic import SyntheticSequence


def epoch_generator(seed, epoch, stream=0):
    """The generator every per-epoch draw comes from: a function of (seed, epoch, stream) alone."""
    return torch.Generator().manual_seed((int(seed) * 1000003 + int(epoch)) * 31 + int(stream))


def draw_specs(g, visible, n_frames, epoch_samples, epoch_repeats, sample_size):
    """One epoch's SampleSpecs from generator ``g``.  visible: (sequence, object) -> frame indices in which the object is visible;
    n_frames: sequence -> length.  ``epoch_samples`` pairs are drawn if > 0 (all of them otherwise, in sorted order); per pair and
    repeat, frame 0 is drawn from the visible frames and the others without replacement from the rest of the sequence."""
    pairs = sorted(visible)
    if epoch_samples > 0:
        pick = torch.randperm(len(pairs), generator=g)[:epoch_samples].tolist()
        pairs = [pairs[i] for i in pick]
    specs = []
    for name, obj in pairs:
        for _ in range(epoch_repeats):
            vis = visible[(name, obj)]
            first = vis[int(torch.randint(len(vis), (1,), generator=g))]
            others = [t for t in range(n_frames[name]) if t != first]
            rest = [others[i] for i in torch.randperm(len(others), generator=g)[:sample_size - 1].tolist()]
            specs.append(SampleSpec(name, int(obj), [first] + rest, first))
    return specs


class TrainingDataset(torch.utils.data.Dataset):
    """Sampling over sequences that offer ``name``, ``obj_ids``, ``images[t]`` (3,H,W) uint8 and ``gt[t]`` (1,H,W) uint8 label maps."""
    MIN_PIXELS = 100           # an object smaller than this in a frame counts as not visible there

    def __init__(self, sequences, epoch_repeats=1, epoch_samples=0, min_seq_length=4, sample_size=3, seed=0):
        if sample_size < 2:
            raise ValueError('sample_size must be at least 2 (frame 0 fits the target model, the others train), got %d' % sample_size)
        self.sequences = {s.name: s for s in sequences if len(s.images) >= max(min_seq_length, sample_size)}
        self.epoch_repeats, self.epoch_samples, self.sample_size, self.seed = int(epoch_repeats), int(epoch_samples), int(sample_size), int(seed)
        self.visible = {}        # (sequence, object) -> frame indices in which the object is visible
        for s in self.sequences.values():
            for obj in s.obj_ids:
                frames = [t for t in range(len(s.images)) if int((s.gt[t] == obj).sum()) >= self.MIN_PIXELS]
                if frames:
                    self.visible[(s.name, obj)] = frames
        if not self.visible:
            raise ValueError('no (sequence, object) pair is long enough and visible')
        self.specs = []
        self.set_epoch(0)

    def set_epoch(self, epoch):
        self.specs = draw_specs(epoch_generator(self.seed, epoch), self.visible, {n: len(s.images) for n, s in self.sequences.items()},
                                self.epoch_samples, self.epoch_repeats, self.sample_size)

    def __len__(self):
        return len(self.specs)

    def __getitem__(self, i):
        spec = self.specs[i]
        seq = self.sequences[spec.seq_name]
        images = [seq.images[t].cpu() for t in spec.frames]
        labels = [(seq.gt[t] == spec.obj_id).to(torch.uint8).cpu() for t in spec.frames]
        return images, labels, spec.encoded()


class SyntheticTrainingDataset(TrainingDataset):
    """Sample sets over ``n_sequences`` seeded lib.synthetic.SyntheticSequence clips (textured rectangles moving over a low-pass
    background) with the reference datasets' knobs."""

    def __init__(self, n_sequences=8, n_frames=8, size=(480, 854), n_objects=1, epoch_repeats=1, epoch_samples=0, min_seq_length=4,
                 sample_size=3, seed=0):
        seqs = [SyntheticSequence('synth%03d' % k, n_frames, tuple(size), n_objects, seed=1000 * int(seed) + k + 1) for k in range(n_sequences)]
        super().__init__(seqs, epoch_repeats, epoch_samples, min_seq_length, sample_size, seed)


# ----------------------------------------------------------------------------------------------------------------------------------
# File-backed sample sets
# ----------------------------------------------------------------------------------------------------------------------------------
def default_meta_file(name, workspace='workspace'):
    """Where a sample set keeps its occlusion table unless told otherwise: under the training workspace (train.py --workspace), never
    inside the package."""
    return Path(workspace) / 'meta' / ('%s_meta.pth' % name)


class FileTrainingDataset(torch.utils.data.Dataset):
    """Sample sets over a dataset on disk: ``jpeg_path/<sequence>/<frame>.jpg`` and palette PNGs ``anno_path/<sequence>/<frame>.png``.

    Occlusion table (the reference's ``<name>_meta.pth``): ``dict(frame_names={seq: [stem, ...]}, occlusions={seq: (N, M) bool array})``,
    N annotated frames, M = highest object id + 1, column 0 the background, True = occluded.  It is read from ``meta_file`` when that
    exists -- also one written by the reference, whose table is then used as it is -- and otherwise computed from the annotations
    (per-frame, per-object pixel counts; ``_occlusions`` of the subclass) and written there.  The file is a function of the annotations,
    the sequence list and ``overrides``: delete it, or name another, when any of them changes."""
    MIN_PIXELS = TrainingDataset.MIN_PIXELS

    def __init__(self, name, jpeg_path, anno_path, sequences, epoch_repeats, epoch_samples, min_seq_length, sample_size, seed, meta_file):
        if sample_size < 2:
            raise ValueError('sample_size must be at least 2 (frame 0 fits the target model, the others train), got %d' % sample_size)
        self.name, self.jpeg_path, self.anno_path = name, Path(jpeg_path), Path(anno_path)
        self.sequences = list(sequences)
        self.epoch_repeats, self.epoch_samples, self.sample_size, self.seed = int(epoch_repeats), int(epoch_samples), int(sample_size), int(seed)
        self.meta_file = Path(meta_file) if meta_file is not None else default_meta_file(name)
        meta = self.load_meta()
        self.frame_names, self.occlusions = meta['frame_names'], meta['occlusions']
        self.visible, self.n_frames = {}, {}
        for seq in self.sequences:
            occ = np.asarray(self.occlusions[seq], dtype=bool)
            if occ.shape[0] < max(min_seq_length, self.sample_size):
                continue
            self.n_frames[seq] = occ.shape[0]
            for obj in range(1, occ.shape[1]):                       # objects that are not occluded in every frame
                frames = np.flatnonzero(~occ[:, obj]).tolist()
                if frames:
                    self.visible[(seq, obj)] = frames
        if not self.visible:
            raise ValueError('%s: no (sequence, object) pair is long enough and visible' % name)
        self.specs = []
        self.set_epoch(0)

    # ---- occlusion table ----
    def pixel_counts(self, seq):
        """(frame stems, (N, M) int64 pixel counts per annotated frame and label id) of one sequence, decoded on the host."""
        from PIL import Image
        files = sorted((self.anno_path / seq).glob('*.png'))
        if not files:
            raise FileNotFoundError('%s: no annotations under %s' % (self.name, self.anno_path / seq))
        counts = np.stack([np.bincount(np.asarray(Image.open(f), dtype=np.uint8).ravel(), minlength=256) for f in files])
        return [f.stem for f in files], counts[:, :int(np.flatnonzero(counts.sum(0)).max()) + 1]

    def _occlusions(self, seq, counts):
        raise NotImplementedError

    def load_meta(self):
        if self.meta_file.exists():
            meta = torch.load(self.meta_file, map_location='cpu', weights_only=False)      # (numpy arrays inside)
            missing = [s for s in self.sequences if s not in meta['occlusions']]
            if missing:
                raise KeyError('%s lacks the sequences %s' % (self.meta_file, missing[:3]))
            return meta
        print('Computing occlusions for %s under %s' % (self.name, self.anno_path), flush=True)
        frame_names, occlusions = {}, {}
        for seq in sorted(self.sequences):
            frame_names[seq], counts = self.pixel_counts(seq)
            occlusions[seq] = np.asarray(self._occlusions(seq, counts), dtype=bool)
        meta = dict(frame_names=frame_names, occlusions=occlusions)
        self.meta_file.parent.mkdir(parents=True, exist_ok=True)
        tmp = self.meta_file.with_name('%s.%d.tmp' % (self.meta_file.name, os.getpid()))
        torch.save(meta, tmp)
        tmp.replace(self.meta_file)                                    # (a reader never sees a torn file)
        return meta

    # ---- sampling ----
    def set_epoch(self, epoch):
        self.specs = draw_specs(epoch_generator(self.seed, epoch), self.visible, self.n_frames, self.epoch_samples, self.epoch_repeats,
                                self.sample_size)

    def __len__(self):
        return len(self.specs)

    def __getitem__(self, i):
        """(images, labels, meta) at the frames' NATIVE size: uint8 (3,h,w) and raw label ids (1,h,w); see the module docstring."""
        from .image import imread
        spec = self.specs[i]
        stems = [self.frame_names[spec.seq_name][t] for t in spec.frames]
        images = [imread(self.jpeg_path / spec.seq_name / (s + '.jpg')) for s in stems]
        images = [im if im.shape[0] == 3 else im[:1].expand(3, -1, -1).contiguous() for im in images]      # (grey-scale JPEGs)
        labels = [imread(self.anno_path / spec.seq_name / (s + '.png')) for s in stems]
        return images, labels, spec.encoded()


def load_overrides(overrides):
    """``overrides`` of DAVISDataset: a dict, the path of a JSON file holding one, or None."""
    if overrides is None:
        return {}
    if not isinstance(overrides, dict):
        overrides = json.load(open(overrides))
    known = {'threshold', 'never_occluded', 'visible'}
    for seq, o in overrides.items():
        if not isinstance(o, dict) or set(o) - known:
            raise ValueError('occlusion overrides of %r: expected a dict with keys from %s, got %r' % (seq, sorted(known), o))
    return overrides


class DAVISDataset(FileTrainingDataset):
    """DAVIS 2017 train: ``JPEGImages/480p``, ``Annotations/480p``, ``ImageSets/2017/train.txt`` under ``dset_path``.

    An object is occluded in a frame when it covers fewer than MIN_PIXELS pixels there, or less than ``threshold`` (0.25) of the most it
    covers anywhere in the sequence: count / (max_count + 0.001) < threshold.  ``overrides`` (a dict or a JSON file) adjusts the
    fraction rule per sequence -- the hard minimum always applies:
        {"<sequence>": {"threshold": x}}                              another fraction
        {"<sequence>": {"never_occluded": true}}                      no fraction rule
        {"<sequence>": {"visible": [[f0, f1, obj_or_null], ...]}}     frames f0 <= t < f1 (f1 null: to the end) pass the fraction rule,
                                                                      for one object id or (null) all
    No per-sequence table ships with this package."""
    THRESHOLD = 0.25

    def __init__(self, dset_path, epoch_repeats=1, epoch_samples=0, min_seq_length=4, sample_size=3, seed=0, meta_file=None, overrides=None):
        root = Path(dset_path).expanduser()
        sequences = [s.strip() for s in open(root / 'ImageSets' / '2017' / 'train.txt') if s.strip()]
        self.overrides = load_overrides(overrides)
        super().__init__('davis', root / 'JPEGImages' / '480p', root / 'Annotations' / '480p', sequences, epoch_repeats, epoch_samples,
                         min_seq_length, sample_size, seed, meta_file)

    def _occlusions(self, seq, counts):
        o = self.overrides.get(seq, {})
        peak = counts.max(axis=0)
        if o.get('never_occluded'):
            occ = np.zeros(counts.shape, dtype=bool)
        else:
            occ = (counts / (peak + 0.001) < float(o.get('threshold', self.THRESHOLD))) | (peak == 0)
        for f0, f1, obj in o.get('visible', ()):
            occ[f0:f1, slice(None) if obj is None else obj] = False
        return occ | (counts < self.MIN_PIXELS)


class YouTubeVOSDataset(FileTrainingDataset):
    """YouTube-VOS train: ``train/JPEGImages``, ``train/Annotations`` under ``dset_path``; every annotated sequence, or the ids listed
    in ``sequences_file`` (one per line; the reference's 'jjtrain' list is a file of its repository and is not copied here).  An object
    is occluded in a frame when it covers fewer than MIN_PIXELS pixels there."""

    def __init__(self, dset_path, epoch_samples=4000, epoch_repeats=1, min_seq_length=4, sample_size=3, year=2018, seed=0, meta_file=None,
                 sequences_file=None):
        root = Path(dset_path).expanduser()
        anno = root / 'train' / 'Annotations'
        if sequences_file is not None:
            sequences = sorted(s.strip() for s in open(sequences_file) if s.strip())
        else:
            sequences = sorted(p.name for p in anno.glob('*') if p.is_dir())
        super().__init__('ytvos%s' % year, root / 'train' / 'JPEGImages', anno, sequences, epoch_repeats, epoch_samples, min_seq_length,
                         sample_size, seed, meta_file)

    def _occlusions(self, seq, counts):
        return counts < self.MIN_PIXELS


def raw_collate(batch):
    """collate_fn for native-size samples: (images, labels, meta) with images[t][b] / labels[t][b] the frame t of sample b, left as
    the tensors the dataset returned (sizes differ within a batch), meta the list of encoded SampleSpecs."""
    n = len(batch[0][0])
    return [[s[0][t] for s in batch] for t in range(n)], [[s[1][t] for s in batch] for t in range(n)], [s[2] for s in batch]


class DeviceFrameResizer:
    """Batch transform between ``raw_collate`` and ``TrainerModel.forward``: packs the batch's raw frames back to back into a pinned
    staging buffer (and the label maps into a second one), copies each to the device once and resamples all frames / all labels to
    ``size`` with one launch each (ops.resize_frames_u8 / resize_labels_u8).  Returns (images, labels, meta) with images[t] a (B,3,H,W)
    and labels[t] a (B,1,H,W) uint8 device tensor, the label the sample's object as 0 / 1.

    Mode per frame, the reference's rule (lib/training_datasets.py:186-187): 'area' when H / h < 1 or the frame belongs to a DAVIS sample
    set, else 'cubic'.  ``datasets``: the FileTrainingDatasets in use; sequences of those named 'davis' always take 'area'."""

    def __init__(self, size=(480, 854), device='cuda:0', datasets=()):
        self.size, self.device = (int(size[0]), int(size[1])), normalize_device(device)
        self.area_sequences = {s for d in datasets if getattr(d, 'name', None) == 'davis' for s in d.sequences}
        self._staging = [None, None]                               # pinned buffers: frames, labels
        self._copied = None                                        # event behind the last batch's copies

    def mode(self, seq_name, h):
        return 'area' if self.size[0] / h < 1.0 or seq_name in self.area_sequences else 'cubic'

    def _pack(self, which, tensors, last):
        """tensors -> (pinned staging buffer holding them back to back, (n,4) table of rows (offset, h, w, last[k]))."""
        total = sum(t.numel() for t in tensors)
        buf = self._staging[which]
        if buf is None or buf.numel() < total:
            buf = self._staging[which] = torch.empty(total, dtype=torch.uint8).pin_memory()
        rows, off = [], 0
        for t, v in zip(tensors, last):
            if t.dtype != torch.uint8 or t.dim() != 3:
                raise TypeError('DeviceFrameResizer: expected uint8 (C,h,w) frames, got %s %s' % (t.dtype, tuple(t.shape)))
            buf[off:off + t.numel()].copy_(t.reshape(-1))
            rows.append((off, t.shape[1], t.shape[2], v))
            off += t.numel()
        return buf[:total], torch.tensor(rows, dtype=torch.int64)

    def __call__(self, batch):
        from .. import ops
        images, labels, meta = batch
        specs = SampleSpec.from_encoded(meta)
        T, B = len(images), len(meta)
        frames = [images[t][b] for t in range(T) for b in range(B)]
        maps = [labels[t][b] for t in range(T) for b in range(B)]
        with torch.cuda.device(self.device):
            if self._copied is not None:
                self._copied.synchronize()                         # the staging buffers are free again
            modes = [ops.RESIZE_MODES[self.mode(specs[b].seq_name, images[t][b].shape[1])] for t in range(T) for b in range(B)]
            host_im, table_im = self._pack(0, frames, modes)
            host_lb, table_lb = self._pack(1, maps, [specs[b].obj_id for _ in range(T) for b in range(B)])
            dev_im, dev_lb = host_im.to(self.device, non_blocking=True), host_lb.to(self.device, non_blocking=True)
            self._copied = torch.cuda.Event()
            self._copied.record()
            out_im = ops.resize_frames_u8(dev_im, table_im, 3, self.size)
            out_lb = ops.resize_labels_u8(dev_lb, table_lb, self.size)
        return [out_im[t * B:(t + 1) * B] for t in range(T)], [out_lb[t * B:(t + 1) * B] for t in range(T)], meta
