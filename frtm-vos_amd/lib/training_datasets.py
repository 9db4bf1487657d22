"""Sample sets for refiner training (counterpart of the reference's lib/training_datasets.py, written against its interface).

The contract a training dataset fulfils, and ``TrainerModel.forward`` consumes after the DataLoader's default collate:

    dataset[i] -> (images, labels, meta)
        images   ``sample_size`` uint8 tensors (3,H,W): frames of ONE sequence; frame 0 is one in which the object is visible (the target
                 model is fitted on it), the others are drawn from the rest of the sequence without replacement
        labels   ``sample_size`` uint8 tensors (1,H,W): the chosen object relabelled to 1, everything else 0
        meta     ``SampleSpec(seq_name, obj_id, frames, frame0_id).encoded()``: the identity under which the target model is cached

    len(dataset)            samples per epoch: (sequence, object) pairs (``epoch_samples`` of them drawn at random if > 0) times ``epoch_repeats``
    dataset.set_epoch(e)    redraws the samples from a generator seeded by (seed, e): a resumed run draws what an uninterrupted one would

``SyntheticTrainingDataset`` is the one implementation that needs no files.  File-backed DAVIS / YouTube-VOS training sets (with their
occlusion metadata) are not implemented."""
import torch

from ..model.training_model import SampleSpec
from .synthetic import SyntheticSequence


def epoch_generator(seed, epoch, stream=0):
    """The generator every per-epoch draw comes from: a function of (seed, epoch, stream) alone."""
    return torch.Generator().manual_seed((int(seed) * 1000003 + int(epoch)) * 31 + int(stream))


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
        g = epoch_generator(self.seed, epoch)
        pairs = sorted(self.visible)
        if self.epoch_samples > 0:
            pick = torch.randperm(len(pairs), generator=g)[:self.epoch_samples].tolist()
            pairs = [pairs[i] for i in pick]
        self.specs = []
        for name, obj in pairs:
            n = len(self.sequences[name].images)
            for _ in range(self.epoch_repeats):
                vis = self.visible[(name, obj)]
                first = vis[int(torch.randint(len(vis), (1,), generator=g))]
                others = [t for t in range(n) if t != first]
                rest = [others[i] for i in torch.randperm(len(others), generator=g)[:self.sample_size - 1].tolist()]
                self.specs.append(SampleSpec(name, int(obj), [first] + rest, first))

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
