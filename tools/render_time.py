"""What drawing the answer costs: ops.render_frames (csrc/frame_render.hip) on 1080 x 1920 frames, alone, against a torch composition of the
same operation, and behind StreamPool.step().  Writes profiles/render_time.txt.  Not part of bench.py.  The method is that of
tools/decoder_frames_time.py: device events around synchronised work, the arms taking turns in one process after warm-up, medians with
[min .. max] of at least 16 repetitions.

  (a) the launch alone: NV12 and planar RGB; a label map and a K = 3 mask stack; hard, edge and soft; bytes moved against 6.3 TB/s
  (b) the caller's alternative: NV12 / RGB -> float -> blend by the label's colour and opacity -> back (box chroma), written with torch ops
  (c) StreamPool ticks of 1, 4 and 8 streams of 1080p decoder frames at working_size=(480, 854): step() alone against step() + render()
      into caller-provided surfaces

No decoder was available: the surfaces are made from synthetic frames by a torch encoder.

    python tools/render_time.py"""
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
OUT = os.path.join(ROOT, 'profiles', 'render_time.txt')
WS = (480, 854)
SRC = (1080, 1920)
PITCH, CODED = 2048, 1088
ROUNDS = 16
WARM = 9                       # ticks before the first timed one: past the first filter re-solve (frame 8)
REPS = 50                      # launches back to back between two events
HBM = 6.3e12                   # achievable HBM rate, bytes / s
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


def surface(data):
    return ops.DecoderFrame(data, SRC[0], SRC[1], pitch=PITCH, uv_offset=PITCH * CODED)


def torch_render_nv12(surf, labels, table, out):
    """The hard rule on an NV12 surface as a caller writes it with torch ops (even h and w): float Y,U,V with replicated chroma, the
    label's colour and opacity gathered, the blend, the chroma averaged back over its block."""
    h, w = SRC
    y = surf[:PITCH * h].view(h, PITCH)[:, :w].float()
    uv = surf[PITCH * CODED:PITCH * CODED + PITCH * (h // 2)].view(h // 2, PITCH)[:, :w].reshape(h // 2, w // 2, 2).float()
    s = torch.cat([y[..., None], uv.repeat_interleave(2, 0).repeat_interleave(2, 1)], dim=-1)
    st = table[labels.long()].float()
    o = s + (st[..., :3] - s) * (st[..., 3:] / 255.0)
    out[:PITCH * h].view(h, PITCH)[:, :w] = o[..., 0].round().to(torch.uint8)
    c = torch.nn.functional.avg_pool2d(o[..., 1:].permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0)
    out[PITCH * CODED:PITCH * CODED + PITCH * (h // 2)].view(h // 2, PITCH)[:, :w] = c.round().to(torch.uint8).reshape(h // 2, w)
    return out


def torch_render_rgb(frame, labels, table, out):
    st = table[labels.long()].float().permute(2, 0, 1)
    s = frame.float()
    out.copy_((s + (st[:3] - s) * (st[3:] / 255.0)).round().to(torch.uint8))
    return out


def modules():
    def refiner(chans):
        torch.manual_seed(1)
        return make_score_following_refiner(SegNetwork(1, 64, chans, True).eval())
    params = Parameters(None, fast=False, device=DEV, feature_extractor='resnet101')
    params.refiner_factory = refiner
    return params, params.get_model().eval()


def verdict(a, b, med, ev):
    d = med[b] - med[a]
    slower = a if med[a] >= med[b] else b
    spread = max(ev[slower]) - min(ev[slower])
    word = 'inside the spread' if abs(d) <= spread else ('%s is FASTER' % (b if d < 0 else a))
    return '%s - %s = %+.3f against a max - min of %.3f in the slower arm (%s): %s' % (b, a, d, spread, slower, word)


def sources(n_frames):
    """Two synthetic 1080p sequences as (surface, labels, new objects) per frame."""
    out = []
    for k in range(2):
        seq = SyntheticSequence('r%d' % k, n_frames, SRC, 2, seed=90 + k)
        seq.preload(DEV)
        out.append([(encode(image), labels, new) for image, labels, new in seq])
        seq.release()
    return out


def launches(srcs):
    (h, w) = SRC
    surf, labels = srcs[0][0][0], srcs[0][0][1]                       # the first frame: the one that comes with a label map
    labels = (labels if torch.is_tensor(labels) else torch.as_tensor(labels)).to(DEV).reshape(h, w).to(torch.uint8).contiguous()
    ids = sorted(set(labels.unique().tolist()) | {0})[:3]
    while len(ids) < 3:
        ids.append(max(ids) + 1)
    lut = torch.tensor(ids, dtype=torch.uint8, device=DEV)
    stack = torch.stack([(labels == i).float() * 0.9 for i in ids]).contiguous()
    planar = ops.frames_to_rgb_u8(surf, torch.tensor([surface(surf).row(0)]), SRC)[0].contiguous()
    frames = {'nv12': surface(surf), 'rgb': planar}
    outs = {'nv12': surface(torch.zeros_like(surf)), 'rgb': torch.empty_like(planar)}
    styles = {'hard': ops.RenderStyle(), 'edge': ops.RenderStyle(edge_alpha=255), 'soft': ops.RenderStyle(soft=True)}
    samples = {'nv12': h * w * 3 // 2, 'rgb': 3 * h * w}
    arms, nbytes = {}, {}
    for f in ('nv12', 'rgb'):
        for ans, mode in (('labels', 'hard'), ('labels', 'edge'), ('K=3 stack', 'hard'), ('K=3 stack', 'edge'), ('K=3 stack', 'soft')):
            a, l = (labels, None) if ans == 'labels' else (stack, lut)
            name = 'render_frames %-4s %-9s %s' % (f, ans, mode)
            arms[name] = (lambda f=f, a=a, l=l, mode=mode: ops.render_frames([frames[f]], [a], styles[mode], luts=[l], out=[outs[f]]))
            nbytes[name] = 2 * samples[f] + a.numel() * a.element_size()
    tables = {f: styles['hard'].device_table(DEV, frames['nv12'].format if f == 'nv12' else 0) for f in ('nv12', 'rgb')}
    touts = {'nv12': torch.zeros_like(surf), 'rgb': torch.empty_like(planar)}
    arms['torch composition nv12 labels    hard'] = lambda: torch_render_nv12(surf, labels, tables['nv12'], touts['nv12'])
    arms['torch composition rgb  labels    hard'] = lambda: torch_render_rgb(planar, labels, tables['rgb'], touts['rgb'])
    nbytes['torch composition nv12 labels    hard'] = nbytes['render_frames nv12 labels    hard']
    nbytes['torch composition rgb  labels    hard'] = nbytes['render_frames rgb  labels    hard']
    # the composition and the kernel state the same operation: within one level of each other (the composition rounds half to even, in float)
    ref = ops.render_frames([frames['nv12']], [labels], styles['hard'], out=[outs['nv12']])[0].data
    d = (torch_render_nv12(surf, labels, tables['nv12'], touts['nv12'])[:PITCH * h].view(h, PITCH)[:, :w].int() - ref[:PITCH * h].view(h, PITCH)[:, :w].int()).abs().max()
    assert int(d) <= 1, int(d)
    reps = {name: (10 if name.startswith('torch') else REPS) for name in arms}
    for name, fn in arms.items():                                     # warm-up of every shape
        for _ in range(5):
            fn()
    ev = {name: [] for name in arms}
    for _ in range(ROUNDS):                                            # the arms take turns
        for name, fn in arms.items():
            d, _ = timed(lambda: [fn() for _ in range(reps[name])])
            ev[name].append(d * 1e3 / reps[name])
    say('')
    say('## (a), (b) one %d x %d frame into a caller-provided surface: us per call, %d calls back to back between two events (torch: 10),' % (SRC + (REPS,)))
    say('## median [min .. max] of %d rounds, the arms taking turns; bytes = samples read + answer read + samples written, against %.1f TB/s' % (ROUNDS, HBM / 1e12))
    say('%-42s %-33s %10s %10s %8s' % ('call', 'us', 'MB moved', 'us at HBM', 'share'))
    for name in arms:
        bound = nbytes[name] / HBM * 1e6
        say('%-42s %-33s %10.2f %10.2f %7.0f%%' % (name, fmt(ev[name]), nbytes[name] / 1e6, bound, 100 * bound / statistics.median(ev[name])))
    med = {k: statistics.median(v) for k, v in ev.items()}
    for f in ('nv12', 'rgb '):
        say('# us: ' + verdict('torch composition %s labels    hard' % f, 'render_frames %s labels    hard' % f, med, ev))
    say('# a call is ops.render_frames as a caller makes it on surfaces it has rendered before: the rows built, their uploaded table found, ONE launch;')
    say('# at a few us it is bound by launch latency and the host, not by bytes: the share column says how far from the byte bound it is, nothing more.')


def pool_ticks(params, model, srcs, S):
    mods = (model.augmenter, model.feature_extractor, params.disc_params, model.refiner, DEV)
    arms = ('step', 'step+render')
    pools = {k: StreamPool(*mods, max_streams=S, trunk_lanes=params.trunk_lanes, working_size=WS) for k in arms}
    sids = {k: [p.open() for _ in range(S)] for k, p in pools.items()}
    mine = {sid: surface(torch.zeros_like(srcs[0][0][0])) for sid in sids['step+render']}
    style = ops.RenderStyle(edge_alpha=255)
    ev, solve = ({k: [] for k in arms} for _ in range(2))

    def tick(name, t):
        pool, frames = pools[name], {}
        for i, sid in enumerate(sids[name]):
            surf, labels, new = srcs[i % 2][t]
            image = surface(surf)
            if len(new) > 0:
                torch.manual_seed(0)
                pool.initialize(sid, image, labels, new)
            frames[sid] = image
        out = pool.step(frames)
        if name == 'step+render' and out:
            pool.render(frames, style, out=mine)
        return out
    t = 0
    while len(ev[arms[0]]) < ROUNDS:
        for name in [arms[(t + i) % 2] for i in range(2)]:
            if t <= WARM:
                tick(name, t)
                continue
            d, out = timed(lambda: tick(name, t))
            assert len(out) == S
            (solve if t % 8 == 0 else ev)[name].append(d)
        t += 1
    assert pools['step'].render_launches == 0 and pools['step+render'].render_launches == t - 1
    say('')
    say('## (c) StreamPool, S = %d streams of %d x %d decoder frames, 2 objects each, working size %d x %d' % ((S,) + SRC + WS))
    say('%-12s %-33s %s' % ('arm', 'tick ms (device events)', 're-solve ticks ms'))
    med = {k: statistics.median(ev[k]) for k in arms}
    for k in arms:
        say('%-12s %-33s %s' % (k, fmt(ev[k]), ' '.join('%.3f' % v for v in solve[k])))
    say('# ms: ' + verdict('step', 'step+render', med, ev))
    for k, p in pools.items():
        for sid in sids[k]:
            p.close(sid)
    del pools
    torch.cuda.empty_cache()


def main():
    prop = torch.cuda.get_device_properties(0)
    say('# Rendering the answer onto 1080p frames (NV12: pitch %d, coded height %d; planar RGB); %s (%s, %d CUs); %s' % (
        PITCH, CODED, prop.name, getattr(prop, 'gcnArchName', '?').split(':')[0], prop.multi_processor_count, time.strftime('%Y-%m-%d')))
    say('# (c): ResNet-101, full iteration schedule, memory 80, synthetic sequences, score-following stand-in refiner, working_size=(%d, %d);' % WS)
    say('# timed ticks start after %d warm-up ticks; median [min .. max] of the %d ticks without a filter re-solve.' % (WARM, ROUNDS))
    say("# One arm beats another only when the medians differ by more than the slower arm's own max - min.")
    say('# No decoder was available: the surfaces come from a torch encoder, no real surface was fed in.')
    params, model = modules()
    srcs = sources(1 + WARM + ROUNDS + ROUNDS // 7 + 3)
    launches(srcs)
    for S in (1, 4, 8):
        pool_ticks(params, model, srcs, S)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


if __name__ == '__main__':
    with torch.no_grad():
        main()
