"""Time the bf16x1 refiner training mode (SegNetwork.train_precision = 'bf16x1') against the fp32 one on the shapes of a B = 16, 480x854 RN101
training step.  Writes profiles/bf16x1_refiner_train_time.txt.

  (1) per shape: frtm_conv_wgrad (fp32 MFMA) against frtm_conv_wgrad_bf16x1 for every 3x3 weight-gradient shape of the step, and the forward conv
      of the one input-gradient pair the inference table lacks (32 -> 64, the head conv1's input gradient);
  (2) the routing verdicts: a pair is routed from its smallest measured launch from which every measured launch's bf16 median beats the fp32
      median by more than the fp32 arm's spread (max - min); the tables printed here are the ones ops.py carries;
  (3) the refiner's forward + backward under both precisions (with the tables of (2) installed for the run), and TrainerModel.forward +
      optimiser step as tools/train_step_time.py times it.
All arms alternate in one process after warm-up; device events around every repetition; median [min .. max].

    python tools/bf16x1_refiner_train_time.py                 the table
    python tools/bf16x1_refiner_train_time.py --kernels-only  three bf16x1 training passes and nothing else: the run to put under
                                                              rocprofv3 --kernel-trace --stats
    python tools/bf16x1_refiner_train_time.py --stats-csv F   append the backward's per-kernel breakdown from that run's kernel_trace.csv
    python tools/bf16x1_refiner_train_time.py --curves A B    append the loss / IoU trajectories of two train.py logs (fp32, bf16x1)
"""
import copy
import csv
import json
import os
import statistics
import sys
import time
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd import ops  # noqa: E402
from frtm_vos_amd.model.seg_network import SegNetwork  # noqa: E402

DEV = 'cuda:0'
OUT = os.path.join(ROOT, 'profiles', 'bf16x1_refiner_train_time.txt')
REPS = 24
B = 16
HW = (480, 854)
RN101 = OrderedDict(layer5=2048, layer4=1024, layer3=512, layer2=256)
LEVELS = ((15, 27), (30, 54), (60, 107), (120, 214))
PAIRS = ((64, 64), (65, 65), (65, 64), (64, 32))          # (cin, cout) of the refiner's 3x3 convs
HEAD = (240, 428)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(arms, reps=REPS, warm=3):
    for _ in range(warm):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn))
    return t


def blocks(n, h, w, cout):
    return n * ((h + 7) // 8) * ((w + 7) // 8) * ((cout + 31) // 32)


def verdicts(rows):
    """rows: (cin, cout, blocks, fp32 times, bf16 times) -> {(cin, cout): fewest blocks from which every measured launch is faster}."""
    table = {}
    for pair in sorted({(r[0], r[1]) for r in rows}):
        mine = sorted((r for r in rows if (r[0], r[1]) == pair), key=lambda r: r[2])
        first = None
        for r in reversed(mine):
            f, b = r[3], r[4]
            if statistics.median(f) - statistics.median(b) > max(f) - min(f):
                first = r[2]
            else:
                break
        if first is not None:
            table[pair] = first
    return table


def wgrad_rows():
    g = torch.Generator().manual_seed(0)
    rows = []
    say('(1) 3x3 weight gradients, B = %d: frtm_conv_wgrad (fp32) against frtm_conv_wgrad_bf16x1; us, median [min .. max] of %d alternating rounds' % (B, REPS))
    say('%-26s %8s %30s %30s %9s %s' % ('shape', 'blocks', 'fp32 us', 'bf16x1 us', 'fp32/bf16', 'rel. rms of bf16x1 - fp32'))
    shapes = [(cin, cout, h, w) for (h, w) in LEVELS for (cin, cout) in PAIRS] + [(64, 32) + HEAD]
    for cin, cout, h, w in shapes:
        x = torch.relu(torch.randn(B, cin, h, w, generator=g)).to(DEV)
        dy = torch.randn(B, cout, h, w, generator=g).to(DEV)
        t = alternate(OrderedDict(f=lambda: ops.conv_wgrad(dy, x, 3), b=lambda: ops.conv_wgrad(dy, x, 3, bf16x1=True)))
        a, b = ops.conv_wgrad(dy, x, 3)[0], ops.conv_wgrad(dy, x, 3, bf16x1=True)[0]
        rel = float((a - b).double().pow(2).mean().sqrt() / a.double().pow(2).mean().sqrt())
        f, bb = [1e3 * v for v in t['f']], [1e3 * v for v in t['b']]
        nb = blocks(B, h, w, cout)
        rows.append((cin, cout, nb, f, bb))
        say('%-26s %8d %10.1f [%8.1f .. %8.1f] %10.1f [%8.1f .. %8.1f] %9.2f %.2e' % (
            '%d x %d->%d @ %dx%d' % (B, cin, cout, h, w), nb, statistics.median(f), min(f), max(f), statistics.median(bb), min(bb), max(bb),
            statistics.median(f) / statistics.median(bb), rel))
        del x, dy
    return rows


def dgrad_rows():
    """The head conv1's input gradient: a forward 3x3 conv 32 -> 64 at 240x428, weights packed per call as the training pass does."""
    from frtm_vos_amd.model.refiner_train import _Runner
    g = torch.Generator().manual_seed(1)
    net = SegNetwork(1, 64, {'layer4': 8}, False).to(DEV)
    net.bf16_min_blocks = 0
    rows = []
    say('(1b) input gradient of the head conv1 (a forward conv 32 -> 64, packed per call): fp32 route against FRTM_WLAYOUT_BF16X1_3X3')
    for cin, cout, h, w in ((32, 64) + HEAD,):
        dy = torch.randn(B, cin, h, w, generator=g).to(DEV)
        wt = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(DEV)
        net.train_precision = 'fp32'
        Rf = _Runner(net, DEV)
        net.train_precision = 'bf16x1'
        Rb = _Runner(net, DEV)
        net.train_precision = 'fp32'
        t = alternate(OrderedDict(f=lambda: Rf.conv(dy, wt), b=lambda: Rb.conv(dy, wt)))
        f, bb = [1e3 * v for v in t['f']], [1e3 * v for v in t['b']]
        nb = blocks(B, h, w, cout)
        rows.append((cin, cout, nb, f, bb))
        say('%-26s %8d %10.1f [%8.1f .. %8.1f] %10.1f [%8.1f .. %8.1f] %9.2f' % (
            '%d x %d->%d @ %dx%d' % (B, cin, cout, h, w), nb, statistics.median(f), min(f), max(f), statistics.median(bb), min(bb), max(bb),
            statistics.median(f) / statistics.median(bb)))
    return rows


def refiner_inputs():
    g = torch.Generator().manual_seed(1)
    feats = {}
    for i, (L, c) in enumerate(RN101.items()):
        s = 32 >> i
        feats[L] = torch.relu(torch.randn(B, c, (HW[0] + s - 1) // s, (HW[1] + s - 1) // s, generator=g)).to(DEV)
    scores = torch.randn(B, 1, feats['layer4'].shape[2], feats['layer4'].shape[3], generator=g).to(DEV)
    dl = torch.randn(B, 1, *HW, generator=g).to(DEV) * 1e-3
    return scores, feats, dl


def pass_arms():
    torch.manual_seed(0)
    nets = OrderedDict(fp32=SegNetwork(1, 64, RN101, True).to(DEV).train())
    nets['bf16x1'] = copy.deepcopy(nets['fp32'])
    nets['bf16x1'].train_precision = 'bf16x1'
    scores, feats, dl = refiner_inputs()

    def step(net):
        for p in net.parameters():
            p.grad = None
        net.forward_train(scores, feats, HW).backward(dl)
    return OrderedDict((k, (lambda n=n: step(n))) for k, n in nets.items())


def trainer_arms():
    import tempfile
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.fused_adam import FusedAdam
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    from frtm_vos_amd.model.augmenter import ImageAugmenter
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    from frtm_vos_amd.model.training_model import SampleSpec, TrainerModel
    P = Parameters(None, fast=True, device=DEV, feature_extractor='resnet101')
    P.disc_params.update(memory_size=20, init_iters=(3, 5), update_iters=(3,), c_channels=32)
    ext = ResnetFeatureExtractor('resnet101').to(DEV)
    seqs = [SyntheticSequence('t%d' % k, 3, HW, 1, seed=50 + k) for k in range(B)]
    images = [torch.stack([s.images[t] for s in seqs]).to(DEV) for t in range(3)]
    labels = [torch.stack([(s.gt[t] == 1).to(torch.uint8) for s in seqs]).to(DEV) for t in range(3)]
    meta = [SampleSpec('t%d' % k, 1, [0, 1, 2], 0).encoded() for k in range(B)]
    cache = dict(path=tempfile.mkdtemp(prefix='tmcache'), enable=True, read_only=False)
    torch.manual_seed(1)
    init = SegNetwork(1, 64, RN101, True).to(DEV)
    arms = OrderedDict()
    for name in ('fp32', 'bf16x1'):
        net = copy.deepcopy(init)
        net.train_precision = name
        m = TrainerModel(ImageAugmenter(P.aug_params), ext, P.disc_params, net, batch_size=B, tmodel_cache=cache, device=DEV,
                         refiner_backend='hip', loss_backend='hip')
        opt = FusedAdam(net.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-5, amsgrad=True)

        def step(m=m, opt=opt):
            opt.zero_grad()
            st = m(images, labels, meta)
            opt.step()
            return st
        arms[name] = step
    return arms


def ratio_row(what, t):
    f, b = t['fp32'], t['bf16x1']
    say('%-40s fp32 %8.2f ms [%8.2f .. %8.2f]   bf16x1 %8.2f ms [%8.2f .. %8.2f]   fp32 / bf16x1 = %.3f' % (
        what, statistics.median(f), min(f), max(f), statistics.median(b), min(b), max(b), statistics.median(f) / statistics.median(b)))


def main():
    prop = torch.cuda.get_device_properties(0)
    say('# bf16x1 refiner training mode (csrc/conv_wgrad_bf16x1.hip, csrc/conv3x3_bf16x1.hip) against fp32; %s (%s, %d CUs); %s' % (
        prop.name, getattr(prop, 'gcnArchName', '?').split(':')[0], prop.multi_processor_count, time.strftime('%Y-%m-%d')))
    say('# operands: ReLU\'d normal activations, normal output gradients; device events around each repetition, arms alternating in one process')
    with torch.enable_grad():
        rows = wgrad_rows()
        wtable = verdicts(rows)
        say('# routing verdicts (weight gradient): faster = fp32 median - bf16x1 median > the fp32 arm\'s max - min; a (Cin, Cout) pair is routed')
        say('# from the block count of its smallest measured launch from which every measured launch is faster; unmeasured pairs stay fp32')
        say('BF16X1_WGRAD_ROUTES = %r' % (wtable,))
        have = dict(ops.BF16X1_WGRAD_ROUTES)
        say('ops.BF16X1_WGRAD_ROUTES as compiled in: %r   %s' % (have, '(this run\'s)' if have == wtable else (
            '(the same pairs, no count below this run\'s: the larger count of the runs taken -- a verdict at the smallest, host-bound launches '
            'flips with one outlier of the fp32 arm)' if set(have) == set(wtable) and all(have[k] >= wtable[k] for k in have) else '<-- DIFFERS from this run')))
        drows = dgrad_rows()
        dtable = verdicts(drows)
        say('input-gradient pairs this run would add to BF16X1_3X3_ROUTES: %r (compiled in: %r)' % (
            dtable, {k: v for k, v in ops.BF16X1_3X3_ROUTES.items() if k in {(r[0], r[1]) for r in drows}}))
        ops.BF16X1_WGRAD_ROUTES.clear()
        ops.BF16X1_WGRAD_ROUTES.update(wtable)
        ops.BF16X1_3X3_ROUTES.update(dtable)
        say('(3) whole passes, B = %d, %dx%d, RN101 taps, use_bn=True, train mode, the tables above installed; %d rounds' % (B, HW[0], HW[1], REPS))
        ratio_row('refiner forward + backward', alternate(pass_arms()))
        torch.cuda.empty_cache()
        ratio_row('TrainerModel.forward + FusedAdam step', alternate(trainer_arms(), warm=2))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


def kernels_only():
    arms = pass_arms()
    for _ in range(3):
        arms['bf16x1']()
    torch.cuda.synchronize()


def append_stats(path):
    groups = {}
    for r in csv.DictReader(open(path)):
        k = r.get('Kernel_Name', '').replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        groups.setdefault(k, []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    total = sum(sum(v) for v in groups.values())
    with open(OUT, 'a') as f:
        f.write('# per kernel, from a separate `rocprofv3 --kernel-trace --stats -- python tools/bf16x1_refiner_train_time.py --kernels-only` run:\n'
                '# three bf16x1 training passes (forward + backward), all kernels, sorted by total time; share of the GPU time of the run\n')
        f.write('%-60s %6s %12s %10s %7s\n' % ('kernel', 'calls', 'total us', 'median us', 'share'))
        for k, ns in sorted(groups.items(), key=lambda kv: -sum(kv[1]))[:24]:
            f.write('%-60s %6d %12.1f %10.2f %6.1f%%\n' % (k[:60], len(ns), sum(ns) / 1e3, statistics.median(ns) / 1e3, 100.0 * sum(ns) / total))
    print('appended %d kernels to %s' % (len(groups), OUT))


def append_curves(a, b):
    runs = [[json.loads(s) for s in open(p) if s.strip()] for p in (a, b)]
    with open(OUT, 'a') as f:
        f.write('# accuracy at workload level: python -m frtm_vos_amd.train --dset synthetic at the same seed, fp32 against --refiner-precision bf16x1;\n'
                '# ONE run each, %d epochs of the synthetic set (epoch means of the loss and of the IoU); not a gate\n' % min(len(r) for r in runs))
        f.write('%6s %12s %12s %12s %12s\n' % ('epoch', 'fp32 loss', 'bf16x1 loss', 'fp32 IoU', 'bf16x1 IoU'))
        n = min(len(r) for r in runs)
        for i in sorted(set(list(range(0, n, max(n // 20, 1))) + [n - 1])):
            r0, r1 = runs[0][i], runs[1][i]
            f.write('%6d %12.5f %12.5f %12.4f %12.4f\n' % (r0['epoch'], r0['stats/loss'], r1['stats/loss'], r0['stats/accuracy'], r1['stats/accuracy']))
    print('appended the curves to', OUT)


if __name__ == '__main__':
    if '--kernels-only' in sys.argv:
        with torch.enable_grad():
            kernels_only()
    elif '--stats-csv' in sys.argv:
        append_stats(sys.argv[sys.argv.index('--stats-csv') + 1])
    elif '--curves' in sys.argv:
        i = sys.argv.index('--curves')
        append_curves(sys.argv[i + 1], sys.argv[i + 2])
    else:
        main()
