"""Time the refiner's training step (forward + backward) at upstream train.py's shape: HIP (SegNetwork.forward_train) against the PyTorch
definition (forward_torch: MIOpen convolutions, PyTorch batch norm / interpolate / autograd), alternated in one process.
B = 16 frames of 480x854, RN101 tap widths, use_bn=True, compat head, train mode.  Writes profiles/refiner_train_time.txt.

    python tools/refiner_train_time.py [--batch 16] [--steps 20] [--warmup 3]
"""
import argparse
import os
import statistics
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

CHANS = OrderedDict(layer5=2048, layer4=1024, layer3=512, layer2=256)


def flops_per_sample(Hh, Ww, oc=64):
    """Algorithmic forward FLOPs (2 per multiply-add) of the convolutions, from the shapes."""
    tot, lv = 0.0, {}
    for i, (L, c) in enumerate(CHANS.items()):
        s = 32 >> i
        hw = ((Hh + s - 1) // s) * ((Ww + s - 1) // s)
        f = 2 * hw * (c * oc + oc * oc + 9 * (oc + 1) ** 2 * 2 + 9 * (oc + 1) * oc         # TSE reduce, transform
                      + 2 * (oc * oc + 2 * 9 * oc * oc))                                    # RRB1, RRB2
        lv[L] = f
        tot += f
    h4, w4 = (Hh + 3) // 4, (Ww + 3) // 4
    conv1 = 2 * (2 * h4) * (2 * w4) * 9 * oc * (oc // 2)
    conv2 = 2 * Hh * Ww * 9 * (oc // 2)
    return tot + conv1 + conv2, lv, conv1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', choices=['hip', 'torch'], default=None, help='time one path only (for a rocprofv3 kernel trace)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'refiner_train_time.txt'))
    a = ap.parse_args()
    from frtm_vos_amd.model.seg_network import SegNetwork
    dev = 'cuda:0'
    B, Hh, Ww = a.batch, 480, 854
    torch.manual_seed(0)
    net = SegNetwork(1, 64, CHANS, True).to(dev).train()
    g = torch.Generator().manual_seed(1)
    feats = {}
    for i, (L, c) in enumerate(CHANS.items()):
        s = 32 >> i
        feats[L] = torch.relu(torch.randn(B, c, (Hh + s - 1) // s, (Ww + s - 1) // s, generator=g)).to(dev)
    scores = torch.randn(B, 1, feats['layer4'].shape[2], feats['layer4'].shape[3], generator=g).to(dev)
    dl = torch.randn(B, 1, Hh, Ww, generator=g).to(dev) * 1e-3

    def step(hip):
        for p in net.parameters():
            p.grad = None
        out = net.forward_train(scores, feats, (Hh, Ww)) if hip else net.forward_torch(scores, feats, (Hh, Ww))
        out.backward(dl)

    def timed(hip):
        torch.cuda.synchronize()
        t = time.perf_counter()
        step(hip)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t)
    paths = [True, False] if a.only is None else [a.only == 'hip']
    for _ in range(a.warmup):
        for hip in paths:
            step(hip)
    ts = {hip: [] for hip in paths}
    for _ in range(a.steps):
        for hip in paths:
            ts[hip].append(timed(hip))
    fl, lv, conv1 = flops_per_sample(Hh, Ww)
    lines = ['refiner training step (forward + backward), B = %d, %dx%d, RN101 taps, use_bn=True, compat head, train mode' % (B, Hh, Ww),
             'median over %d steps after %d warm-up steps, the two paths alternated in one process' % (a.steps, a.warmup),
             'algorithmic conv FLOPs: forward %.1f GFLOP per sample (%s; head conv1 %.1f), backward ~2x'
             % (fl / 1e9, ', '.join('%s %.1f' % (L, f / 1e9) for L, f in lv.items()), conv1 / 1e9)]
    for hip in paths:
        m = statistics.median(ts[hip])
        lines.append('%-28s median %8.1f ms  min %8.1f ms  max %8.1f ms  -> %.1f TFLOP/s (3x forward FLOPs)'
                     % ('HIP forward_train' if hip else 'PyTorch forward_torch', m, min(ts[hip]), max(ts[hip]), 3 * fl * B / m / 1e9))
    txt = '\n'.join(lines) + '\n'
    print(txt)
    if a.only is None:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        open(a.out, 'w').write(txt)


if __name__ == '__main__':
    main()
