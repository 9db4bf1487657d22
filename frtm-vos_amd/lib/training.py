"""The training driver (counterpart of the reference's lib/training.py, written against its interface): epochs over a sample-set
dataset, one ``zero_grad / model(*batch) / step`` per batch, ``scheduler.step()`` per epoch, checkpoints and a log.

Checkpoints are ``<checkpoints_path>/<name>/<name>_ep%04d.pth`` with the keys name, epoch, stats, model, optimizer, scheduler.
``model`` is ``model.state_dict()``: for a TrainerModel the refiner under the 'refiner.' prefix, which is what
``python -m frtm_vos_amd.evaluate --model`` reads, so a training checkpoint is an inference checkpoint as it is.  ``stats`` is a plain dict
of floats (the epoch's means).  The log is ``<log_path>/<name>/log.jsonl``, one JSON object per epoch; TensorBoard scalars are written as
well when ``torch.utils.tensorboard`` can be imported, and not missed otherwise.

Everything random about an epoch (the samples drawn, their order) comes from generators seeded by (seed, epoch): a run resumed from
a checkpoint sees the batches an uninterrupted run would."""
import json
import time
from pathlib import Path

import torch
from torch.utils.data import ConcatDataset, DataLoader

from .training_datasets import epoch_generator


class AverageMeter:
    def __init__(self):
        self.val, self.sum, self.count = 0.0, 0.0, 0

    def update(self, v):
        self.val = float(v)
        self.sum += self.val
        self.count += 1

    @property
    def avg(self):
        return self.sum / max(self.count, 1)


class Trainer:

    def __init__(self, name, model, optimizer, scheduler, dataset, checkpoints_path, log_path, max_epochs, batch_size, num_workers=0,
                 load_latest=True, save_interval=5, stats_to_print=('stats/loss', 'stats/accuracy', 'stats/lr', 'stats/fcache_hits'),
                 seed=0, collate_fn=None, batch_transform=None):
        """dataset: one sample-set dataset (lib/training_datasets.py) or a list of them (concatenated).
        collate_fn: the DataLoader's collate step (None: the default one); batch_transform: a callable applied to every collated batch
        before ``model(*batch)`` (None: the batch as it is).  The file-backed sample sets need both: raw_collate and a DeviceFrameResizer."""
        self.name, self.model, self.optimizer, self.scheduler = name, model, optimizer, scheduler
        self.datasets = list(dataset) if isinstance(dataset, (list, tuple)) else [dataset]
        self.checkpoints_path = Path(checkpoints_path) / name
        self.checkpoints_path.mkdir(exist_ok=True, parents=True)
        self.log_path = Path(log_path) / name
        self.epoch = 0
        self.max_epochs, self.batch_size, self.num_workers, self.save_interval = int(max_epochs), int(batch_size), int(num_workers), int(save_interval)
        self.stats_to_print, self.seed = tuple(stats_to_print), int(seed)
        self.collate_fn, self.batch_transform = collate_fn, batch_transform
        self.stats = {}
        self._tb = None
        if load_latest:
            found = sorted(self.checkpoints_path.glob('%s_ep*.pth' % name))
            if found:
                self.load_checkpoint(found[-1])

    def checkpoint_file(self, epoch=None):
        return self.checkpoints_path / ('%s_ep%04d.pth' % (self.name, self.epoch if epoch is None else epoch))

    def load_checkpoint(self, file):
        print('Loading checkpoint', file)
        ckpt = torch.load(file, map_location='cpu')
        self.epoch = int(ckpt['epoch'])
        self.stats = dict(ckpt['stats'])
        self.model.load_state_dict(ckpt['model'])
        self.optimizer.load_state_dict(ckpt['optimizer'])
        self.scheduler.load_state_dict(ckpt['scheduler'])
        print('Starting epoch', self.epoch + 1)

    def save_checkpoint(self):
        ckpt = dict(name=self.name, epoch=self.epoch, stats={k: float(v) for k, v in self.stats.items()}, model=self.model.state_dict(),
                    optimizer=self.optimizer.state_dict(), scheduler=self.scheduler.state_dict())
        tmp = self.checkpoint_file().with_suffix('.tmp')
        torch.save(ckpt, tmp)
        tmp.replace(self.checkpoint_file())            # (a reader never sees a torn file)

    def _loader(self, epoch):
        for d in self.datasets:
            if hasattr(d, 'set_epoch'):
                d.set_epoch(epoch)
        dset = self.datasets[0] if len(self.datasets) == 1 else ConcatDataset(self.datasets)
        return DataLoader(dset, batch_size=self.batch_size, num_workers=self.num_workers, shuffle=True, pin_memory=torch.cuda.is_available(),
                          generator=epoch_generator(self.seed, epoch, stream=1), collate_fn=self.collate_fn)

    def _log(self, seconds):
        self.log_path.mkdir(exist_ok=True, parents=True)
        with open(self.log_path / 'log.jsonl', 'a') as f:
            f.write(json.dumps(dict(epoch=self.epoch, seconds=seconds, **self.stats)) + '\n')
        if self._tb is None:
            try:
                from torch.utils.tensorboard import SummaryWriter
                self._tb = SummaryWriter(str(self.log_path))
            except Exception:                          # not installed: the JSON-lines file is the log
                self._tb = False
        if self._tb:
            for k, v in self.stats.items():
                self._tb.add_scalar(k, v, self.epoch)

    def train(self):
        for epoch in range(self.epoch + 1, self.max_epochs + 1):
            self.epoch = epoch
            meters = {}
            loader = self._loader(epoch)
            t_epoch = t0 = time.time()
            for i, batch in enumerate(loader, 1):
                self.optimizer.zero_grad()
                if self.batch_transform is not None:
                    batch = self.batch_transform(batch)
                stats = dict(self.model(*batch))
                self.optimizer.step()
                stats['stats/lr'] = self.scheduler.get_last_lr()[0]
                for k, v in stats.items():
                    meters.setdefault(k, AverageMeter()).update(v)
                now = time.time()
                shown = ', '.join('%s=%.5f (%.5f)' % (k[6:] if k.startswith('stats/') else k, m.val, m.avg)
                                  for k, m in meters.items() if k in self.stats_to_print)
                print('%d: %d/%d, sps=%.2f, %s' % (epoch, i, len(loader), self.batch_size / max(now - t0, 1e-9), shown), flush=True)
                t0 = now
            self.scheduler.step()
            self.stats = {k: m.avg for k, m in meters.items()}
            if self.epoch % self.save_interval == 0:
                self.save_checkpoint()
            self._log(time.time() - t_epoch)
        print('%s done' % self.name)
