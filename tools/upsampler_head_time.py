"""Device time of the refiner head's tail, compat vs bicubic, on one GPU in one run (record: profiles/).

    python tools/upsampler_head_time.py [--frames 8] [--objects 2] [--size 480x854] [--reps 40] [--iters 20] [--out FILE]

Both heads end the same way: frtm_tap_mix forms conv2's nine tap maps from conv1's 32 channels at the 2x layer2 resolution, then one
kernel resamples them to the image and applies the 3x3 taps -- frtm_project_tail (compat: 2x polyphase + bilinear) or
frtm_project_tail_bicubic (bicubic resize).  Each repetition times `iters` back-to-back launches of each kernel between device events,
the two heads alternating; the record keeps the median and the spread over the repetitions.  Inputs are seeded; both tails run on
the same tap maps.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--objects', type=int, default=2)
    ap.add_argument('--size', default='480x854')
    ap.add_argument('--reps', type=int, default=40)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from frtm_vos_amd import _hip as H
    from frtm_vos_amd.model.seg_network import bicubic_tail_fits
    assert torch.cuda.is_available(), 'needs a GPU'
    dev = 'cuda:0'
    Ho, Wo = (int(v) for v in a.size.lower().split('x'))
    n = a.frames * a.objects
    h, w = 2 * ((Ho + 3) // 4), 2 * ((Wo + 3) // 4)              # conv1's output: 2x the layer2 map
    assert bicubic_tail_fits(h, w, Ho, Wo)
    g = torch.Generator().manual_seed(0)
    y = torch.relu(torch.randn(n, 32, h, w, generator=g)).to(dev)
    w2 = (torch.randn(1, 32, 3, 3, generator=g) * 0.2).to(dev)
    b2 = torch.tensor([0.1], device=dev)
    eye9 = torch.eye(9, device=dev).contiguous()
    ym = torch.empty(n, 9, h, w, device=dev)
    out = torch.empty(n, 1, Ho, Wo, device=dev)
    launches = {
        'tap_mix': lambda: H.call('frtm_tap_mix', H.ptr(y), n, 32, h * w, H.ptr(w2), H.ptr(ym)),
        'tail_compat': lambda: H.call('frtm_project_tail', H.ptr(ym), n, 9, h, w, H.ptr(eye9), H.ptr(b2), Ho, Wo, H.ptr(out)),
        'tail_bicubic': lambda: H.call('frtm_project_tail_bicubic', H.ptr(ym), n, 9, h, w, H.ptr(eye9), H.ptr(b2), Ho, Wo, H.ptr(out)),
    }
    for f in launches.values():                                  # warm-up (code objects loaded, clocks up)
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in launches}
    for r in range(a.reps):
        order = ['tap_mix', 'tail_compat', 'tail_bicubic'] if r % 2 == 0 else ['tap_mix', 'tail_bicubic', 'tail_compat']
        for k in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                launches[k]()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1000.0 / a.iters)
    med = {k: statistics.median(v) for k, v in times.items()}
    res = dict(window='%d frames x %d objects' % (a.frames, a.objects), image=[Ho, Wo], conv1_map=[n, 32, h, w], reps=a.reps, iters=a.iters,
               median_us={k: round(v, 2) for k, v in med.items()},
               min_us={k: round(min(v), 2) for k, v in times.items()}, max_us={k: round(max(v), 2) for k, v in times.items()},
               head_compat_us=round(med['tap_mix'] + med['tail_compat'], 2), head_bicubic_us=round(med['tap_mix'] + med['tail_bicubic'], 2),
               mb_tap_mix=round((n * 32 + n * 9) * h * w * 4 / 1e6, 1), mb_tail=round((n * 9 * h * w + n * Ho * Wo) * 4 / 1e6, 1),
               device=torch.cuda.get_device_name(0))
    res['ratio_bicubic_over_compat'] = round(res['head_bicubic_us'] / res['head_compat_us'], 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
