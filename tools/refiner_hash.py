"""sha256 of what the refiner's two HIP paths (SegNetwork._forward_hip, SegNetwork.forward_train + backward) and the mask merge compute, for an
A/B of two trees that must not differ in a bit:  python tools/refiner_hash.py [package root]   (one process per tree; diff the outputs).

``package root``: the directory that holds frtm_vos_amd.py and a built frtm-vos_amd/ (default: this tree).  The networks and inputs are
_net / _inputs of tests/test_refiner_train_gpu.py of THIS tree either way (SMALL tap widths, oc = 64), use_bn on and off.

Inference, six forms: 2 frames x 2 objects at 480 x 854, 3 frames x 1 object and 1 x 1 (the 3x3 convs of the 120 x 214, 60 x 107 and
30 x 54 levels fall on both sides of the 512 blocks of the Winograd launch rule: 3240 / 896 / 224, 2430 / 672 / 168 and 810 / 224 / 56
blocks); the 2 x 2 maps with image size (240, 427), where the fused tail does not fit and the unfused head runs; the bicubic head where
its fused tail fits and where it does not.  Ragged inference: frames of 1, 3 and 2 objects through an ops.RaggedTable (the table kernels of
csrc/ragged_group.hip), fitting and non-fitting image size.
Training: forward_train + backward at batch 2, train and eval mode, a fitting and a non-fitting image size; the logits, every parameter
gradient and every buffer (BatchNorm running statistics and batch counts).
Merge: ops.track_merge on 2 frames x 3 objects without labels and with the several-object and the one-object decode, ops.track_merge_ragged
on counts (1, 3, 2) and (15, 1); 257 pixels (one partial block) and 480 x 854; masks, counts and labels.
The kernels are deterministic, so one unequal hash is a changed order of operations, not noise."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else ROOT
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, PKG)
import frtm_vos_amd  # noqa: E402
from frtm_vos_amd import _hip as H, ops  # noqa: E402
from frtm_vos_amd.model.seg_network import Upsampler  # noqa: E402
from test_refiner_train_gpu import SMALL, _inputs, _net  # noqa: E402

DEV = 'cuda:0'
assert os.path.dirname(os.path.abspath(frtm_vos_amd.__file__)) == PKG, frtm_vos_amd.__file__


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16]


def inference(use_bn):
    # (frames, objects, image size, head)
    forms = [(2, 2, (480, 854), 'compat'), (3, 1, (480, 854), 'compat'), (1, 1, (480, 854), 'compat'), (2, 2, (240, 427), 'compat'),
             (2, 2, (480, 854), 'bicubic'), (2, 2, (240, 427), 'bicubic')]
    for frames, objects, size, head in forms:
        net = _net(SMALL, use_bn)
        if head == 'bicubic':
            torch.manual_seed(3)
            net.project = Upsampler(64)
        net = net.eval().to(DEV)
        scores, feats = _inputs(SMALL, frames, 480, 854)
        scores = torch.randn(frames * objects, 1, *scores.shape[-2:], generator=torch.Generator().manual_seed(4))
        with torch.no_grad():
            out = net._forward_hip(scores.to(DEV), {L: t.to(DEV) for L, t in feats.items()}, size)
        print('inference use_bn=%d %d x %d -> %s %s head: %s' % (use_bn, frames, objects, size, head, sha(out)))


def ragged_inference(use_bn):
    for size in ((480, 854), (240, 427)):
        table = ops.RaggedTable((1, 3, 2), DEV)
        net = _net(SMALL, use_bn).eval().to(DEV)
        scores, feats = _inputs(SMALL, table.F, 480, 854)
        scores = torch.randn(table.n, 1, *scores.shape[-2:], generator=torch.Generator().manual_seed(4))
        with torch.no_grad():
            out = net._forward_hip(scores.to(DEV), {L: t.to(DEV) for L, t in feats.items()}, size, None, table)
        print('inference use_bn=%d frames of %r objects -> %s: %s' % (use_bn, table.counts, size, sha(out)))


def merges():
    lut = torch.tensor([0, 3, 5, 9], dtype=torch.uint8, device=DEV)
    for HW in (257, 480 * 854):
        logits = (torch.randn(2 * 3, 1, 1, HW, generator=torch.Generator().manual_seed(11)) * 3).to(DEV)
        for decode in (None, 'several', 'one'):
            masks, counts = torch.empty(2, 4, 1, HW, device=DEV), torch.zeros(2, 4, dtype=torch.int32, device=DEV)
            labels = None if decode is None else torch.zeros(2, 1, 1, HW, dtype=torch.uint8, device=DEV)
            ops.track_merge(logits, 2, 3, masks, labels, None if decode is None else lut, decode == 'one', counts)
            tag = 'track_merge 2 x 3, HW = %d, decode %s' % (HW, decode)
            print('%s: masks %s counts %s%s' % (tag, sha(masks), sha(counts), '' if labels is None else ' labels ' + sha(labels)))
        for cnt in ((1, 3, 2), (15, 1)):
            table = ops.RaggedTable(cnt, DEV)
            logits = (torch.randn(table.n, 1, 1, HW, generator=torch.Generator().manual_seed(12)) * 3).to(DEV)
            masks, counts = torch.zeros(table.n + table.F, 1, HW, device=DEV), torch.zeros(table.n + table.F, dtype=torch.int32, device=DEV)
            ops.track_merge_ragged(logits, table, masks, counts)
            print('track_merge_ragged %r, HW = %d: masks %s counts %s' % (cnt, HW, sha(masks), sha(counts)))


def training(use_bn):
    for train in (True, False):
        for size in ((480, 854), (240, 427)):
            net = _net(SMALL, use_bn).to(DEV).train(train)
            scores, feats = _inputs(SMALL, 2, 480, 854)
            dl = torch.randn(2, 1, *size, generator=torch.Generator().manual_seed(9)).to(DEV)
            out = net.forward_train(scores.to(DEV), {L: t.to(DEV) for L, t in feats.items()}, size)
            out.backward(dl)
            tag = 'training use_bn=%d %s -> %s' % (use_bn, 'train' if train else 'eval', size)
            print('%s logits: %s' % (tag, sha(out)))
            for name, p in net.named_parameters():
                print('%s grad %s: %s' % (tag, name, sha(p.grad)))
            for name, b in net.named_buffers():
                print('%s buffer %s: %s' % (tag, name, sha(b)))


H.lib()
print('library:', [ln.split()[-1] for ln in open('/proc/self/maps') if 'libfrtm_hip' in ln][0], file=sys.stderr)      # (stderr: the outputs stay comparable)
for use_bn in (True, False):
    inference(use_bn)
    ragged_inference(use_bn)
    training(use_bn)
merges()
