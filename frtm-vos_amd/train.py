"""Train the refiner (counterpart of the reference's train.py, its hyper-parameters wired onto this package's HIP training step).

``python -m frtm_vos_amd.train NAME [--ftext resnet101|resnet18] [--dev cuda:0] [--dset synthetic|davis|ytvos|davis+ytvos]
[--davis-path DIR] [--ytvos-path DIR] [--ytvos-sequences-file FILE] [--occlusion-overrides FILE] [--num-workers N] [--epochs N]
[--batch-size B] [--workspace DIR] [--batched-scores]``

Per batch: target models fitted on the augmented first frames on the HIP path (or read from the cache under the workspace), the
refiner's forward and backward (``refiner_backend='hip'``), the loss tail (``loss_backend='hip'``) and the AMSGrad step (``FusedAdam``)
on the project's kernels.  Recipe as the reference's: Adam, lr 1e-3, betas (0.9, 0.999), weight_decay 1e-5, amsgrad, StepLR(127, 0.1),
batch 16, three frames per sample, a checkpoint per epoch under ``<workspace>/checkpoints/NAME/`` that ``evaluate.py --model`` reads.

``--dset synthetic`` (the default) trains on generated clips and needs no files.  ``davis``, ``ytvos`` and ``davis+ytvos`` read DAVIS 2017
train / YouTube-VOS train from disk (lib/training_datasets.py): frames are decoded at their native size by the loader and resized to
480 x 854 on the device, a batch per launch (csrc/frame_resize.hip); the occlusion tables are computed on first use and kept under
``<workspace>/meta/``.
"""
import argparse
from pathlib import Path

import torch

from .evaluate import AttrDict


class ModelParameters:
    """The training configuration of the reference (train.py:23-92): 15 augmentations of the first frame, a 32-channel target model
    without pixel weighting, the 64-channel refiner with BatchNorm."""

    def __init__(self, name, feature_extractor='resnet101', device='cuda:0', batch_size=None, tmodel_cache_path=None, trunk_precision='fp32',
                 refiner_precision='fp32', batched_scores=False):
        self.name, self.device, self.batch_size = name, device, batch_size
        self.batched_scores = bool(batched_scores)    # the batch's target models score their frames in one grouped launch (TrainerModel.batched_scores)
        if trunk_precision not in ('fp32', 'bf16x3', 'bf16x1', 'bf16x1_3x3', 'bf16x1_act'):
            raise ValueError("trunk_precision must be 'fp32', 'bf16x3', 'bf16x1', 'bf16x1_3x3' or 'bf16x1_act', got %r" % (trunk_precision,))
        self.trunk_precision = trunk_precision        # the frozen trunk's routed 1x1 convs on bf16 pieces (ResnetFeatureExtractor.precision)
        if refiner_precision not in ('fp32', 'bf16x1'):
            raise ValueError("refiner_precision must be 'fp32' or 'bf16x1', got %r" % (refiner_precision,))
        self.refiner_precision = refiner_precision    # the refiner's training pass: its routed 3x3 convs and weight gradients on bf16 (SegNetwork.train_precision)
        self.feature_extractor = feature_extractor
        self.aug_params = AttrDict(
            num_aug=15, min_px_count=1,
            fg_aug_params=AttrDict(
                rotation=[5, -5, 10, -10, 20, -20, 30, -30, 45, -45], fliplr=[False, False, False, False, True],
                scale=[0.5, 0.7, 1.0, 1.5, 2.0, 2.5], skew=[(0.0, 0.0), (0.0, 0.0), (0.1, 0.1)],
                blur_size=[0.0, 0.0, 0.0, 2.0], blur_angle=[0, 45, 90, 135]),
            bg_aug_params=AttrDict(
                tcenter=[(0.5, 0.5)], rotation=[0, 0, 0], fliplr=[False], scale=[1.0, 1.0, 1.2], skew=[(0.0, 0.0)],
                blur_size=[0.0, 0.0, 1.0, 2.0, 5.0], blur_angle=[0, 45, 90, 135]))
        self.disc_params = AttrDict(
            layer='layer4', in_channels=256 if '18' in feature_extractor else 1024, c_channels=32, out_channels=1,
            init_iters=(5, 10, 10, 10, 10), update_iters=(10,), update_filters=True,
            filter_reg=(1e-5, 1e-4), precond=(1e-5, 1e-4), precond_lr=0.1, CG_forgetting_rate=75,
            memory_size=20, train_skipping=8, learning_rate=0.1, pixel_weighting=None, device=device)
        self.refnet_params = AttrDict(refinement_layers=('layer5', 'layer4', 'layer3', 'layer2'), nchannels=64, use_batch_norm=True)
        self.tmodel_cache = AttrDict(enable=tmodel_cache_path is not None, read_only=False,
                                     path=None if tmodel_cache_path is None else
                                     Path(tmodel_cache_path) / ('%s-c%d' % (feature_extractor, self.disc_params.c_channels)))

    def get_model(self):
        from .model.augmenter import ImageAugmenter
        from .model.feature_extractor import ResnetFeatureExtractor
        from .model.seg_network import SegNetwork
        from .model.training_model import TrainerModel
        augmenter = ImageAugmenter(self.aug_params)
        extractor = ResnetFeatureExtractor(self.feature_extractor, precision=self.trunk_precision).to(self.device)       # weights: FRTM_RESNET_WEIGHTS, else seeded synthetic ones
        p = self.refnet_params
        chans = {L: n for L, n in extractor.get_out_channels().items() if L in p.refinement_layers}
        self.disc_params.in_channels = extractor.get_out_channels()[self.disc_params.layer]
        torch.manual_seed(1)                                       # seeded default init, as evaluate.Parameters.make_refiner
        refiner = SegNetwork(1, p.nchannels, chans, p.use_batch_norm, train_precision=self.refiner_precision).to(self.device)
        return TrainerModel(augmenter, extractor, self.disc_params, refiner, batch_size=self.batch_size, tmodel_cache=self.tmodel_cache,
                            device=self.device, refiner_backend='hip', loss_backend='hip', batched_scores=self.batched_scores)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='Train the FRTM refiner (MI355X-native training step)')
    ap.add_argument('name', help='name of the training session: checkpoint and log sub-directories')
    ap.add_argument('--ftext', default='resnet101', choices=['resnet101', 'resnet18'], help='feature extractor')
    ap.add_argument('--dev', default='cuda:0')
    ap.add_argument('--dset', default='synthetic', choices=['synthetic', 'davis', 'ytvos', 'davis+ytvos'], help='training data')
    ap.add_argument('--davis-path', default=None, help='DAVIS root (JPEGImages/480p, Annotations/480p, ImageSets/2017/train.txt)')
    ap.add_argument('--ytvos-path', default=None, help='YouTube-VOS root (train/JPEGImages, train/Annotations)')
    ap.add_argument('--ytvos-sequences-file', default=None, help='YouTube-VOS sequence ids to train on, one per line (default: all)')
    ap.add_argument('--occlusion-overrides', default=None, help='JSON file of per-sequence DAVIS occlusion overrides')
    ap.add_argument('--num-workers', type=int, default=0, help='DataLoader workers (decoding; the resize runs on the device)')
    ap.add_argument('--epochs', type=int, default=260)
    ap.add_argument('--batch-size', type=int, default=16)
    ap.add_argument('--workspace', default='workspace', help='checkpoints/, logs/ and tmodels_cache/ are created below it')
    ap.add_argument('--synthetic-sequences', type=int, default=32)
    ap.add_argument('--synthetic-size', default='480x854', help='HxW of the synthetic frames')
    ap.add_argument('--trunk-precision', choices=['fp32', 'bf16x3', 'bf16x1', 'bf16x1_3x3', 'bf16x1_act'], default='fp32',
                    help="the frozen trunk's routed 1x1 convs: fp32, three bf16 pieces (fp32-level) or one bf16 piece (NOT fp32-level); "
                         "bf16x1_3x3: one bf16 piece for the routed 3x3 convs as well; bf16x1_act: that, with bf16 storage of the activations between routed convs")
    ap.add_argument('--refiner-precision', choices=['fp32', 'bf16x1'], default='fp32',
                    help="the refiner's training pass: bf16x1 runs the routed 3x3 convs, input and weight gradients on bf16 MFMAs with fp32 "
                         "accumulation (NOT fp32-level; master weights, BatchNorm, 1x1 convs and checkpoints stay fp32)")
    ap.add_argument('--batched-scores', action='store_true',
                    help='score the frames of a batch with all its target models in one grouped launch (ops.target_apply_grouped) instead of one '
                         'projection + filter pass per sample')
    return ap.parse_args(argv)


def file_datasets(args, workspace):
    """The file-backed sample sets ``--dset`` names, with the reference's epoch sizes (train.py:123-125: DAVIS 8 repeats, YouTube-VOS
    4000 samples)."""
    from .lib.training_datasets import DAVISDataset, YouTubeVOSDataset, default_meta_file
    out = []
    for kind in args.dset.split('+'):
        path = {'davis': args.davis_path, 'ytvos': args.ytvos_path}[kind]
        if path is None:
            raise SystemExit('--dset %s needs --%s-path' % (args.dset, kind))
        if kind == 'davis':
            out.append(DAVISDataset(path, epoch_repeats=8, sample_size=3, meta_file=default_meta_file('davis', workspace),
                                    overrides=args.occlusion_overrides))
        else:
            out.append(YouTubeVOSDataset(path, epoch_samples=4000, sample_size=3, meta_file=default_meta_file('ytvos2018', workspace),
                                         sequences_file=args.ytvos_sequences_file))
    return out


def main(argv=None):
    from .lib.fused_adam import FusedAdam
    from .lib.training import Trainer
    from .lib.training_datasets import DeviceFrameResizer, SyntheticTrainingDataset, raw_collate
    args = parse_args(argv)
    ws = Path(args.workspace).expanduser().resolve()
    if torch.device(args.dev).type == 'cuda':
        torch.cuda.set_device(torch.device(args.dev).index or 0)
    hooks = {}
    if args.dset == 'synthetic':
        size = tuple(int(v) for v in args.synthetic_size.lower().split('x'))
        dataset = SyntheticTrainingDataset(n_sequences=args.synthetic_sequences, size=size, sample_size=3)
    else:
        dataset = file_datasets(args, ws)
        hooks = dict(collate_fn=raw_collate, batch_transform=DeviceFrameResizer((480, 854), args.dev, datasets=dataset))
    params = ModelParameters(args.name, feature_extractor=args.ftext, device=args.dev, tmodel_cache_path=ws / 'tmodels_cache',
                             batch_size=args.batch_size, trunk_precision=args.trunk_precision, refiner_precision=args.refiner_precision,
                             batched_scores=args.batched_scores)
    model = params.get_model()
    optimizer = FusedAdam(model.refiner.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-5, amsgrad=True)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=127, gamma=0.1)
    trainer = Trainer(args.name, model, optimizer, scheduler, dataset, checkpoints_path=ws / 'checkpoints', log_path=ws / 'logs',
                      max_epochs=args.epochs, batch_size=args.batch_size, num_workers=args.num_workers, load_latest=True, save_interval=1,
                      **hooks)
    trainer.train()


if __name__ == '__main__':
    main()
