"""What feeding the training step from files costs on the device side: a YouTube-VOS-shaped batch -- 16 samples x 3 frames of 720 x 1280,
with their label maps -- through lib/training_datasets.py: DeviceFrameResizer to 480 x 854.  Writes profiles/frame_resize_time.txt.

Timed separately, device events around every repetition after warm-up: the two host -> device copies from the pinned staging buffers,
the two launches (csrc/frame_resize.hip); with a host clock around a synchronised call: the packing into the staging buffers (host
memcpy) and the whole transform.  The sum of copies and launches is set against the whole training step of batch 16 as measured before
this transform existed (profiles/train_step_time.txt).
    python tools/frame_resize_time.py [--out FILE]"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd import ops  # noqa: E402
from frtm_vos_amd.lib.training_datasets import DeviceFrameResizer  # noqa: E402
from frtm_vos_amd.model.training_model import SampleSpec  # noqa: E402

DEV = 'cuda:0'
OUT = os.path.join(ROOT, 'profiles', 'frame_resize_time.txt')
REPS, WARM = 20, 3
B, T, NATIVE, SIZE = 16, 3, (720, 1280), (480, 854)
STEP_MS = 94.5                 # TrainerModel.forward + FusedAdam step, batch 16, ResNet-101 refiner (profiles/train_step_time.txt, arm B)
HBM_TBS = 6.3                  # achievable HBM rate of the MI355X, TB/s
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def device_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(v):
    return '%8.3f ms [%8.3f .. %8.3f]' % (statistics.median(v), min(v), max(v))


def main():
    out_file = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else OUT
    g = torch.Generator().manual_seed(0)
    images = [[torch.randint(0, 256, (3,) + NATIVE, dtype=torch.uint8, generator=g) for _ in range(B)] for _ in range(T)]
    labels = [[torch.randint(0, 4, (1,) + NATIVE, dtype=torch.uint8, generator=g) for _ in range(B)] for _ in range(T)]
    meta = [SampleSpec('seq%02d' % b, 1 + b % 3, [0, 1, 2], 0).encoded() for b in range(B)]
    batch = (images, labels, meta)
    r = DeviceFrameResizer(SIZE, DEV)
    frames = [images[t][b] for t in range(T) for b in range(B)]
    maps = [labels[t][b] for t in range(T) for b in range(B)]
    t = {k: [] for k in ('pack', 'copy frames', 'copy labels', 'k_resize_frames', 'k_resize_labels', 'whole transform')}
    for rep in range(WARM + REPS):
        keep = rep >= WARM
        ms, (host_im, table_im) = host_ms(lambda: r._pack(0, frames, [ops.RESIZE_MODES['area']] * len(frames)))
        ms2, (host_lb, table_lb) = host_ms(lambda: r._pack(1, maps, [1 + b % 3 for _ in range(T) for b in range(B)]))
        ms_ci, dev_im = device_ms(lambda: host_im.to(DEV, non_blocking=True))
        ms_cl, dev_lb = device_ms(lambda: host_lb.to(DEV, non_blocking=True))
        ms_kf, _ = device_ms(lambda: ops.resize_frames_u8(dev_im, table_im, 3, SIZE))
        ms_kl, _ = device_ms(lambda: ops.resize_labels_u8(dev_lb, table_lb, SIZE))
        ms_all, _ = host_ms(lambda: r(batch))
        if keep:
            for k, v in zip(t, (ms + ms2, ms_ci, ms_cl, ms_kf, ms_kl, ms_all)):
                t[k].append(v)
    mb_im, mb_lb = host_im.numel() / 1e6, host_lb.numel() / 1e6
    out_px = B * T * SIZE[0] * SIZE[1]
    say('# batched resize of native-size frames and labels on HIP (csrc/frame_resize.hip); %s; %s' % (torch.cuda.get_device_name(0), time.strftime('%Y-%m-%d')))
    say('# %d samples x %d frames, %d x %d -> %d x %d, mode area; %d repetitions after %d warm-up rounds: median [min .. max]'
        % (B, T, NATIVE[0], NATIVE[1], SIZE[0], SIZE[1], REPS, WARM))
    say('host: pack into pinned staging (memcpy)        %s' % fmt(t['pack']))
    say('host -> device, frames  %7.1f MB              %s   %.1f GB/s' % (mb_im, fmt(t['copy frames']), mb_im / statistics.median(t['copy frames'])))
    say('host -> device, labels  %7.1f MB              %s   %.1f GB/s' % (mb_lb, fmt(t['copy labels']), mb_lb / statistics.median(t['copy labels'])))
    for name, mb in (('k_resize_frames', mb_im + 3 * out_px / 1e6), ('k_resize_labels', 2 * out_px / 1e6)):
        med = statistics.median(t[name])
        say('%-16s %7.1f MB moved               %s   bound %.3f ms at %.1f TB/s: share %.2f' % (name, mb, fmt(t[name]), mb / HBM_TBS / 1e3, HBM_TBS, mb / HBM_TBS / 1e3 / med))
    total = sum(statistics.median(t[k]) for k in ('copy frames', 'copy labels', 'k_resize_frames', 'k_resize_labels'))
    say('copies + launches (sum of medians)             %8.3f ms = %.1f %% of the %.1f ms training step of batch 16' % (total, 100 * total / STEP_MS, STEP_MS))
    say('whole transform, host clock, synchronised      %s   (packing included)' % fmt(t['whole transform']))
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    with open(out_file, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
