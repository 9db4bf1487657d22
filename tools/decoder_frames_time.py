"""What handing the pool decoder surfaces costs: StreamPool ticks on 1080 x 1920 sources at ``working_size=(480, 854)``, fed three ways.
ResNet-101, the full iteration schedule, 2 objects per stream, synthetic sequences, the score-following stand-in for a trained refiner
(as bench.py).  Writes profiles/decoder_frames_time.txt.  Not part of bench.py.  The method is that of tools/working_size_time.py: device
events around synchronised work, the arms taking turns in one process after warm-up, medians with [min .. max].

  (a) planar   (3, H, W) uint8 tensors: the path the library had before it took decoder frames
  (b) decoder  the same pictures as NV12 surfaces (pitch 2048, coded height 1088) handed over as ops.DecoderFrame
  (c) torch    the same surfaces converted to planar RGB by a composition of torch ops in front of step(): what a caller had to write
  and the kernels alone on one 1080p frame, against their byte counts at 6.3 TB/s

No decoder was available: the surfaces are made from synthetic frames by a torch encoder, and the planar arm gets exactly the planes
the conversion formula makes of them, so all three arms track the same bytes.

    python tools/decoder_frames_time.py"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd import ops  # noqa: E402
from frtm_vos_amd.evaluate import Parameters  # noqa: E402
from frtm_vos_amd.lib.synthetic import SyntheticSequence, make_score_following_refiner  # noqa: E402
from frtm_vos_amd.model.seg_network import SegNetwork  # noqa: E402
from frtm_vos_amd.model.stream_pool import StreamPool  # noqa: E402

DEV = 'cuda:0'
OUT = os.path.join(ROOT, 'profiles', 'decoder_frames_time.txt')
WS = (480, 854)
SRC = (1080, 1920)
PITCH, CODED = 2048, 1088
ROUNDS = 16
WARM = 9                       # ticks before the first timed one: past the first filter re-solve (frame 8)
HBM = 6.3e12                   # achievable HBM rate, bytes / s
Y0, A, RV, GU, GV, BU = 16, 76309, 117489, 13975, 34925, 138438        # 'nv12_bt709' (include/frtm_hip.h)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def fmt(v):
    return '%8.3f [%8.3f .. %8.3f]' % (statistics.median(v), min(v), max(v))


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def encode(rgb):
    """(3, H, W) uint8 on the device -> a flat NV12 surface (BT.709 limited, chroma the mean of its block).  Makes inputs only."""
    h, w = rgb.shape[-2:]
    r, g, b = rgb.float().unbind(0)
    y = 0.2126 * r + 0.7152 * g + 0.0722 * b
    cb, cr = (b - y) / 1.8556, (r - y) / 1.5748
    pool = lambda c: torch.nn.functional.avg_pool2d(c[None, None], 2)[0, 0]
    surf = torch.zeros(PITCH * CODED + PITCH * (h // 2), dtype=torch.uint8, device=rgb.device)
    surf[:PITCH * h].view(h, PITCH)[:, :w] = (16 + 219.0 / 255.0 * y).round().clamp(0, 255).to(torch.uint8)
    uv = torch.stack([128 + 224.0 / 255.0 * pool(cb), 128 + 224.0 / 255.0 * pool(cr)], dim=-1).round().clamp(0, 255).to(torch.uint8)
    surf[PITCH * CODED:].view(h // 2, PITCH)[:, :w] = uv.reshape(h // 2, w)
    return surf


def torch_nv12_to_rgb(surf, h, w):
    """The conversion formula as a caller writes it with torch ops (even h and w): slices, two repeat_interleaves, int32 arithmetic."""
    yy = surf[:PITCH * h].view(h, PITCH)[:, :w].to(torch.int32) - Y0
    uv = surf[PITCH * CODED:PITCH * CODED + PITCH * (h // 2)].view(h // 2, PITCH)[:, :w].reshape(h // 2, w // 2, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, 0).repeat_interleave(2, 1)
    u, v = uv[..., 0], uv[..., 1]
    planes = [A * yy + RV * v, A * yy - GU * u - GV * v, A * yy + BU * u]
    return torch.stack([((p + 32768) >> 16).clamp(0, 255) for p in planes]).to(torch.uint8)


def modules():
    def refiner(chans):
        torch.manual_seed(1)
        return make_score_following_refiner(SegNetwork(1, 64, chans, True).eval())
    params = Parameters(None, fast=False, device=DEV, feature_extractor='resnet101')
    params.refiner_factory = refiner
    return params, params.get_model().eval()


def verdict(a, b, med, ev):
    d, spread = med[b] - med[a], max(ev[a]) - min(ev[a])
    word = 'FASTER' if -d > spread else ('inside the spread' if abs(d) <= spread else 'SLOWER')
    return '%s - %s = %+.3f ms against a spread of %.3f ms in %s: %s' % (b, a, d, spread, a, word)


def sources(n_frames):
    """Two synthetic 1080p sequences as (surface, planar planes of that surface, labels, new objects) per frame."""
    out = []
    for k in range(2):
        seq = SyntheticSequence('d%d' % k, n_frames, SRC, 2, seed=90 + k)
        seq.preload(DEV)
        frames = []
        for image, labels, new in seq:
            surf = encode(image)
            frames.append((surf, torch_nv12_to_rgb(surf, *SRC), labels, new))
        out.append(frames)
        seq.release()
    # the composition and the kernel state the same formula: equal bytes, so the arms track the same pictures
    surf, planar = out[0][1][0], out[0][1][1]
    frame = ops.DecoderFrame(surf, SRC[0], SRC[1], pitch=PITCH, uv_offset=PITCH * CODED)
    assert torch.equal(ops.frames_to_rgb_u8(surf, torch.tensor([frame.row(0)]), SRC)[0], planar)
    return out


def pool_ticks(params, model, srcs, S):
    mods = (model.augmenter, model.feature_extractor, params.disc_params, model.refiner, DEV)
    arms = ('planar', 'decoder', 'torch')
    pools = {k: StreamPool(*mods, max_streams=S, trunk_lanes=params.trunk_lanes, working_size=WS) for k in arms}
    sids = {k: [p.open() for _ in range(S)] for k, p in pools.items()}
    ev, solve = ({k: [] for k in arms} for _ in range(2))

    def tick(name, t):
        pool, frames = pools[name], {}
        for i, sid in enumerate(sids[name]):
            surf, planar, labels, new = srcs[i % 2][t]
            if name == 'decoder':
                image = ops.DecoderFrame(surf, SRC[0], SRC[1], pitch=PITCH, uv_offset=PITCH * CODED)
            elif name == 'torch' and len(new) == 0:
                image = torch_nv12_to_rgb(surf, *SRC)              # inside the timed tick: the caller's conversion is part of its cost
            else:
                image = planar
            if len(new) > 0:
                torch.manual_seed(0)
                pool.initialize(sid, image, labels, new)
            frames[sid] = image
        return pool.step(frames)
    t = 0
    while len(ev[arms[0]]) < ROUNDS:
        order = [arms[(t + i) % 3] for i in range(3)]
        for name in order:
            if t <= WARM:
                tick(name, t)
                continue
            d, out = timed(lambda: tick(name, t))
            assert len(out) == S and all(tuple(m.shape[-2:]) == SRC for m in out.values())
            (solve if t % 8 == 0 else ev)[name].append(d)
        t += 1
    assert pools['decoder'].frame_launches == t - 1 and pools['planar'].frame_launches == 0
    say('')
    say('## StreamPool, S = %d streams of %d x %d sources, 2 objects each, working size %d x %d' % ((S,) + SRC + WS))
    say('%-8s %-33s %s' % ('arm', 'tick ms (device events)', 're-solve ticks ms'))
    med = {k: statistics.median(ev[k]) for k in arms}
    for k in arms:
        say('%-8s %-33s %s' % (k, fmt(ev[k]), ' '.join('%.3f' % v for v in solve[k])))
    say('# ' + verdict('planar', 'decoder', med, ev))
    say('# ' + verdict('torch', 'decoder', med, ev))
    for k, p in pools.items():
        for sid in sids[k]:
            p.close(sid)
    del pools
    torch.cuda.empty_cache()


def kernel_us(fn, reps=50):
    for _ in range(5):
        fn()
    samples = []
    for _ in range(7):
        d, _ = timed(lambda: [fn() for _ in range(reps)])
        samples.append(d * 1e3 / reps)
    return samples


def kernels(srcs):
    say('')
    say('## the kernels alone on one %d x %d frame: us per launch, %d launches back to back between two events, median [min .. max] of 7; bytes / %.1f TB/s'
        % (SRC + (50, HBM / 1e12)))
    say('%-72s %-33s %10s %10s %8s' % ('launch', 'us', 'MB moved', 'us at HBM', 'share'))
    (Hn, Wn), (h, w) = SRC, WS
    surf, planar = srcs[0][1][0], srcs[0][1][1].reshape(-1)

    def row(name, samples, nbytes):
        bound = nbytes / HBM * 1e6
        say('%-72s %-33s %10.2f %10.2f %7.0f%%' % (name, fmt(samples), nbytes / 1e6, bound, 100 * bound / statistics.median(samples)))
    frame = ops.DecoderFrame(surf, Hn, Wn, pitch=PITCH, uv_offset=PITCH * CODED)
    rplan = ops.ResizePlan(torch.tensor([[0, Hn, Wn, ops.RESIZE_MODES['area']]]), DEV)
    fplan = ops.FramePlan(torch.tensor([frame.row(0)]), DEV)
    small, big = torch.empty(1, 3, h, w, dtype=torch.uint8, device=DEV), torch.empty(1, 3, Hn, Wn, dtype=torch.uint8, device=DEV)
    samples = Hn * Wn * 3 // 2
    row("resize_frames_u8 'area', planar 3 x %d x %d -> %d x %d" % (Hn, Wn, h, w), kernel_us(lambda: rplan.frames(planar, 3, WS, out=small)), 3 * Hn * Wn + 3 * h * w)
    row("frames_to_rgb_u8 'area', NV12 %d x %d -> %d x %d (bytes: the samples + out)" % (Hn, Wn, h, w), kernel_us(lambda: fplan.frames(surf, WS, out=small)),
        samples + 3 * h * w)
    row('frames_to_rgb_u8, NV12 %d x %d at its own size (the conversion alone)' % (Hn, Wn), kernel_us(lambda: fplan.frames(surf, SRC, out=big)), samples + 3 * Hn * Wn)
    row('the torch composition, NV12 %d x %d -> planar (bytes: the samples + out)' % (Hn, Wn), kernel_us(lambda: torch_nv12_to_rgb(surf, Hn, Wn), reps=10),
        samples + 3 * Hn * Wn)
    say('# a launch of a few us is bound by launch latency, not by bytes: the share column says how far from the byte bound a launch is, nothing more.')
    say('# the fused kernel converts its footprint once per colour plane (three workgroups read the same Y, U, V bytes) and reads them byte by byte.')


def main():
    prop = torch.cuda.get_device_properties(0)
    say('# Decoder frames (NV12, pitch %d, coded height %d) against planar RGB tensors; %s (%s, %d CUs); %s' % (
        PITCH, CODED, prop.name, getattr(prop, 'gcnArchName', '?').split(':')[0], prop.multi_processor_count, time.strftime('%Y-%m-%d')))
    say('# ResNet-101, full iteration schedule, memory 80, synthetic sequences, score-following stand-in refiner, working_size=(%d, %d).' % WS)
    say('# planar = (3, H, W) uint8 tensors (the path before decoder frames); decoder = the same pictures as ops.DecoderFrame; torch = the surfaces')
    say('# converted by a composition of torch ops in front of step().  Arms take turns in one process; timed ticks start after %d warm-up ticks;' % WARM)
    say("# median [min .. max] of the %d ticks without a filter re-solve.  One arm beats another when the medians differ by more than the other arm's max - min." % ROUNDS)
    say('# No decoder was available: the surfaces come from a torch encoder, no real surface was fed in.')
    params, model = modules()
    srcs = sources(1 + WARM + ROUNDS + ROUNDS // 7 + 3)
    for S in (1, 4, 8):
        pool_ticks(params, model, srcs, S)
    kernels(srcs)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


if __name__ == '__main__':
    with torch.no_grad():
        main()
