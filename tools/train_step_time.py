"""What finishing the training step on HIP costs or saves: the loss tail, the optimiser step and the whole TrainerModel.forward + step,
variant A (HIP refiner pass, torch loss, torch.optim.Adam: the path before csrc/train_step.hip) against variant B (loss_backend='hip',
FusedAdam).  ResNet-101 refiner at 480x854, batch 8 and 16.  Writes profiles/train_step_time.txt.

All arms run in one process, alternating, after warm-up; device events around every repetition.  A second instance of variant A runs as
an arm of its own: the A against A' difference is the spread a B against A difference has to be read against.
    python tools/train_step_time.py                    the table
    python tools/train_step_time.py --kernels-only     a few loss and optimiser launches and nothing else: the run to put under
                                                       rocprofv3 --kernel-trace --stats
    python tools/train_step_time.py --stats-csv FILE   append the two kernels' times from that run's kernel_trace.csv, with their bytes and
                                                       share of the achievable HBM rate"""
import copy
import csv
import os
import statistics
import sys
import time
from collections import OrderedDict

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd.lib.fused_adam import FusedAdam  # noqa: E402
from frtm_vos_amd.model.seg_network import SegNetwork  # noqa: E402
from frtm_vos_amd.model.train_loss import bce_logits_stats, iou_from_counts  # noqa: E402
from frtm_vos_amd.model.training_model import mask_iou  # noqa: E402

DEV = 'cuda:0'
OUT = os.path.join(ROOT, 'profiles', 'train_step_time.txt')
REPS = 24
HBM_TBS = 6.3                  # achievable HBM rate of the MI355X (float4 copy), TB/s
RN101 = OrderedDict(layer5=2048, layer4=1024, layer3=512, layer2=256)
HW = (480, 854)
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
    """arms: name -> callable.  Returns name -> list of ms, the arms taking turns."""
    for _ in range(warm):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            t[k].append(timed(fn))
    return t


def row(what, t, base):
    med = {k: statistics.median(v) for k, v in t.items()}
    cells = '  '.join('%s %8.3f ms [%8.3f .. %8.3f]' % (k, med[k], min(v), max(v)) for k, v in t.items())
    say('%-34s %s   B/%s = %.3f' % (what, cells, base, med['B'] / med[base]))
    return med


def loss_bytes(N, target_bytes):
    return N * HW[0] * HW[1] * (4 + target_bytes + 4)


def refiner():
    torch.manual_seed(1)
    return SegNetwork(1, 64, RN101, True).to(DEV)


def loss_tail_arms(N):
    g = torch.Generator().manual_seed(N)
    z = (torch.randn(N, 1, *HW, generator=g) * 3).to(DEV)
    t8 = (torch.rand(N, 1, *HW, generator=g) < 0.3).to(torch.uint8).to(DEV)
    bce = nn.BCELoss()

    def torch_tail():
        x = z.clone().requires_grad_()
        tf = t8.float()
        pred = torch.sigmoid(x)
        loss = bce(pred, tf)
        loss.backward()
        return loss.detach(), mask_iou(pred.detach(), tf).mean()

    def hip_tail():
        x = z.clone().requires_grad_()
        loss, inter, union = bce_logits_stats(x, t8)
        loss.backward()
        return loss.detach(), iou_from_counts(inter, union).mean()
    with torch.enable_grad():
        a, b = torch_tail(), hip_tail()
    assert abs(float(a[0]) - float(b[0])) < 1e-5 * float(a[0]) and abs(float(a[1]) - float(b[1])) < 1e-6, (a, b)
    return OrderedDict(A=torch_tail, B=hip_tail)


def optimiser_arms():
    arms = OrderedDict()
    for name, cls in (('A', torch.optim.Adam), ('B', FusedAdam)):
        net = refiner()
        g = torch.Generator().manual_seed(3)
        for p in net.parameters():
            p.grad = (torch.randn(p.shape, generator=g) * 1e-2).to(DEV)
        opt = cls(net.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-5, amsgrad=True)
        arms[name] = opt.step
    return arms


def trainer_arms(B):
    """TrainerModel.forward + optimiser step on B sample sets of three 480x854 frames; target models from a pre-filled cache."""
    import tempfile
    from frtm_vos_amd.evaluate import Parameters
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
    init = refiner()
    arms = OrderedDict()
    for name, loss_backend, cls in (('A', 'torch', torch.optim.Adam), ("A'", 'torch', torch.optim.Adam), ('B', 'hip', FusedAdam)):
        net = copy.deepcopy(init)
        m = TrainerModel(ImageAugmenter(P.aug_params), ext, P.disc_params, net, batch_size=B, tmodel_cache=cache, device=DEV,
                         refiner_backend='hip', loss_backend=loss_backend)
        opt = cls(net.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-5, amsgrad=True)

        def step(m=m, opt=opt):
            opt.zero_grad()
            st = m(images, labels, meta)
            opt.step()
            return st
        arms[name] = step
    return arms


def kernels_only():
    for N in (8, 16):
        arms = loss_tail_arms(N)
        for _ in range(5):
            arms['B']()
    opt = optimiser_arms()['B']
    for _ in range(5):
        opt()
    torch.cuda.synchronize()


def append_stats(path):
    n_params = sum(p.numel() for p in SegNetwork(1, 64, RN101, True).parameters())
    groups = {}
    for r in csv.DictReader(open(path)):
        k = r.get('Kernel_Name', '')
        if 'k_bce_logits' in k:
            N = int(r['Grid_Size_Y']) // max(int(r.get('Workgroup_Size_Y', 1) or 1), 1)
            key = ('k_bce_logits<uint8> N=%d' % N, loss_bytes(N, 1))
        elif 'k_adam' in k:
            key = ('k_adam<amsgrad> RN101 refiner', n_params * 4 * 9)
        elif 'k_bce_final' in k or 'k_scale_by' in k:
            key = (k.split('(')[0].split('<')[0], 0)
        else:
            continue
        groups.setdefault(key, []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    with open(OUT, 'a') as f:
        f.write('# per kernel, from a separate `rocprofv3 --kernel-trace --stats -- python tools/train_step_time.py --kernels-only` run;\n'
                '# bytes = what the algorithm has to move (loss: 4 B logit + 1 B target read, 4 B written per pixel; Adam: 5 reads + 4 writes of\n'
                '# 4 B per element); bound = bytes at the achievable HBM rate of %.1f TB/s; share = bound / median time\n' % HBM_TBS)
        f.write('%-34s %6s %10s %10s %10s %10s %10s %7s\n' % ('kernel', 'calls', 'MB', 'bound us', 'median us', 'min us', 'max us', 'share'))
        for (name, nbytes), ns in groups.items():
            med = statistics.median(ns) / 1e3
            bound = nbytes / (HBM_TBS * 1e6)
            f.write('%-34s %6d %10.2f %10.2f %10.2f %10.2f %10.2f %7s\n' % (name, len(ns), nbytes / 1e6, bound, med, min(ns) / 1e3, max(ns) / 1e3,
                                                                             ('%.2f' % (bound / med)) if nbytes else '-'))
    print('appended %d rows to %s' % (len(groups), OUT))


def main():
    prop = torch.cuda.get_device_properties(0)
    say('# the ends of the training step on HIP (csrc/train_step.hip) against the torch tail; %s (%s, %d CUs); %s' % (
        prop.name, getattr(prop, 'gcnArchName', '?').split(':')[0], prop.multi_processor_count, time.strftime('%Y-%m-%d')))
    say('# A = refiner_backend=hip + sigmoid / BCELoss / mask_iou on torch + torch.optim.Adam(amsgrad, wd 1e-5) (the path before this kernel file);')
    say("# A' = a second instance of A; B = loss_backend=hip + FusedAdam.  ResNet-101 refiner, 480x854.  Device events around each repetition,")
    say('# arms alternating in one process after 3 warm-up rounds, %d repetitions each: median [min .. max]' % REPS)
    with torch.enable_grad():
        for N in (8, 16):
            row('(a) loss tail fwd + bwd, N=%d' % N, alternate(loss_tail_arms(N)), 'A')
        row('(b) optimiser step, 116 tensors', alternate(optimiser_arms()), 'A')
        for B in (8, 16):
            t = alternate(trainer_arms(B), warm=2)
            med = row('(c) forward + step, batch %d' % B, t, 'A')
            spread = abs(med["A'"] - med['A']) / med['A']
            say("    A' / A = %.3f: B is %s the A-against-A spread (B - A = %+.3f ms, |A' - A| = %.3f ms)" % (
                med["A'"] / med['A'], 'inside' if abs(med['B'] - med['A']) <= abs(med["A'"] - med['A']) else
                ('faster than A by more than' if med['B'] < med['A'] else 'SLOWER than A by more than'), med['B'] - med['A'], spread * med['A']))
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


if __name__ == '__main__':
    if '--kernels-only' in sys.argv:
        with torch.enable_grad():
            kernels_only()
    elif '--stats-csv' in sys.argv:
        append_stats(sys.argv[sys.argv.index('--stats-csv') + 1])
    else:
        main()
