"""What sending the answer costs: ops.encode_frames (csrc/mask_runs.hip) on a 1080 x 1920 answer, alone and with its copy to the host,
against the two ways a caller has without it, and behind StreamPool.step().  Writes profiles/encode_time.txt.  Not part of bench.py.  The
method is that of tools/object_report_time.py: device events around synchronised work, the arms taking turns in one process after warm-up,
medians with [min .. max] of 16 rounds.

  (a) the call alone: a label map (3 ids) and a K = 3 mask stack; bytes read (the answer twice: counted, then walked again) against 6.3 TB/s
  (b) the call plus MaskRuns.cpu() -- the heads, then runs[:needed] --, against the caller's alternatives on the label map: the same run
      lengths composed of torch ops on the device (transpose, compare with the shifted map, nonzero, diff; one copy per id at the end), and
      the device-to-host copy of the 2 MB label map followed by numpy (timed on the host clock: it is host work; the copy alone is shown too)
  (c) StreamPool ticks of 1, 4 and 8 streams of 1080p frames at working_size=(480, 854): step() alone against step() + encode() with the
      run lengths copied to the host

    python tools/encode_time.py"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd import ops  # noqa: E402
from frtm_vos_amd.evaluate import Parameters  # noqa: E402
from frtm_vos_amd.lib.synthetic import SyntheticSequence, make_score_following_refiner  # noqa: E402
from frtm_vos_amd.model.seg_network import SegNetwork  # noqa: E402
from frtm_vos_amd.model.stream_pool import StreamPool  # noqa: E402

DEV = 'cuda:0'
OUT = os.path.join(ROOT, 'profiles', 'encode_time.txt')
WS = (480, 854)
SRC = (1080, 1920)
ROUNDS = 16
WARM = 9                       # ticks before the first timed one: past the first filter re-solve (frame 8)
REPS = 50                      # calls back to back between two events
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


def host_timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def torch_runs(labels, ids):
    """The run lengths per id as a caller composes them of torch ops on the device -> {id: list}."""
    h, w = labels.shape
    out = {}
    for i in ids:
        bits = (labels == i).t().contiguous().view(-1)                  # column-major
        pos = torch.nonzero(bits[1:] != bits[:-1]).view(-1) + 1
        edge = torch.cat([pos.new_zeros(1), pos, pos.new_full((1,), h * w)])
        runs = (edge[1:] - edge[:-1]).cpu().tolist()
        out[i] = ([0] if bool(bits[0]) else []) + runs
    return out


def numpy_runs(labels, ids):
    """The device-to-host copy of the label map, then the same lists with numpy."""
    lab = labels.cpu().numpy()
    out = {}
    for i in ids:
        bits = (lab == i).flatten(order='F')
        pos = np.flatnonzero(bits[1:] != bits[:-1]) + 1
        runs = np.diff(np.concatenate([[0], pos, [bits.size]])).tolist()
        out[i] = ([0] if bits[0] else []) + runs
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
    """Two synthetic 1080p sequences as (image, labels, new objects) per frame."""
    out = []
    for k in range(2):
        seq = SyntheticSequence('o%d' % k, n_frames, SRC, 2, seed=90 + k)
        seq.preload(DEV)
        out.append([(image, labels, new) for image, labels, new in seq])
        seq.release()
    return out


def calls(srcs):
    (h, w) = SRC
    labels = srcs[0][0][1]                                              # the first frame: the one that comes with a label map
    labels = (labels if torch.is_tensor(labels) else torch.as_tensor(labels)).to(DEV).reshape(h, w).to(torch.uint8).contiguous()
    ids = sorted(set(labels.unique().tolist()) | {0})[:3]
    while len(ids) < 3:
        ids.append(max(ids) + 1)
    lut = torch.tensor(ids, dtype=torch.uint8, device=DEV)
    stack = torch.stack([(labels == i).float() * 0.9 for i in ids]).contiguous()
    coded = {'labels': ops.encode_frames([labels], ids=[ids]), 'stack': ops.encode_frames([stack], luts=[lut])}
    # the three ways state the same lists
    want = numpy_runs(labels, ids)
    assert coded['labels'].counts(0) == want == torch_runs(labels, ids) and coded['stack'].counts(0) == want
    needed = sum(len(c) for c in want.values())
    arms = {
        'encode_frames labels (3 ids)': lambda: ops.encode_frames([labels], ids=[ids], out=coded['labels']),
        'encode_frames K=3 stack': lambda: ops.encode_frames([stack], luts=[lut], out=coded['stack']),
        'encode_frames labels + heads and runs to host': lambda: ops.encode_frames([labels], ids=[ids], out=coded['labels']).cpu(),
        'encode_frames K=3 stack + heads and runs to host': lambda: ops.encode_frames([stack], luts=[lut], out=coded['stack']).cpu(),
        'torch composition labels + lists to host': lambda: torch_runs(labels, ids),
    }
    nbytes = {name: 2 * (stack if 'stack' in name else labels).numel() * (4 if 'stack' in name else 1) for name in arms}
    reps = {name: (REPS if name.startswith('encode_frames') and 'host' not in name else 10) for name in arms}
    for name, fn in arms.items():                                      # warm-up of every shape
        for _ in range(5):
            fn()
    host_arms = {'label map to host (2 MB copy alone)': lambda: labels.cpu(), 'label map to host + numpy': lambda: numpy_runs(labels, ids)}
    for fn in host_arms.values():
        fn()
    ev = {name: [] for name in list(arms) + list(host_arms)}
    for _ in range(ROUNDS):                                             # the arms take turns
        for name, fn in arms.items():
            d, _ = timed(lambda: [fn() for _ in range(reps[name])])
            ev[name].append(d * 1e3 / reps[name])
        for name, fn in host_arms.items():
            d, _ = host_timed(fn)
            ev[name].append(d * 1e3)
    say('')
    say('## (a), (b) one %d x %d answer, 3 objects: us per call, %d calls back to back between two events (arms that end on the host: 10; the two' % (SRC + (REPS,)))
    say('## "label map to host" arms: one call on the host clock), median [min .. max] of %d rounds, the arms taking turns; bytes = the answer read twice, against %.1f TB/s' % (ROUNDS, HBM / 1e12))
    say('%-50s %-36s %10s %10s %8s' % ('call', 'us', 'MB read', 'us at HBM', 'share'))
    for name in arms:
        bound = nbytes[name] / HBM * 1e6
        say('%-50s %-36s %10.2f %10.2f %7.0f%%' % (name, fmt(ev[name]), nbytes[name] / 1e6, bound, 100 * bound / statistics.median(ev[name])))
    for name in host_arms:
        say('%-50s %-36s' % (name, fmt(ev[name])))
    med = {k: statistics.median(v) for k, v in ev.items()}
    say('# us: ' + verdict('torch composition labels + lists to host', 'encode_frames labels + heads and runs to host', med, ev))
    say('# us: ' + verdict('label map to host + numpy', 'encode_frames labels + heads and runs to host', med, ev))
    say('# us: ' + verdict('label map to host (2 MB copy alone)', 'encode_frames labels + heads and runs to host', med, ev))
    say('# us: ' + verdict('encode_frames labels (3 ids)', 'encode_frames K=3 stack', med, ev))
    say('# a call is ops.encode_frames as a caller makes it on buffers it has coded before: the rows built, their uploaded table found, the size of')
    say('# the workspace asked, FOUR enqueued kernels (count, scan of the cells, scan of the slots, store); the share column says how far from the')
    say('# byte bound it is, nothing more.  "+ heads and runs to host" adds MaskRuns.cpu(): two synchronising copies, 512 B and 4 B x needed.')
    say('# this answer: %d run lengths in all (%d B on the way to the host, the label map is %d B); the default capacity K (8 w + 8) = %d leaves %d unused.'
        % (needed, 4 * needed + 512, h * w, coded['labels'].capacity, coded['labels'].capacity - needed))


def pool_ticks(params, model, srcs, S):
    mods = (model.augmenter, model.feature_extractor, params.disc_params, model.refiner, DEV)
    arms = ('step', 'step+encode')
    pools = {k: StreamPool(*mods, max_streams=S, trunk_lanes=params.trunk_lanes, working_size=WS) for k in arms}
    sids = {k: [p.open() for _ in range(S)] for k, p in pools.items()}
    kept = {}
    ev, solve = ({k: [] for k in arms} for _ in range(2))
    seen = dict(ticks=0, overflows=0, most=0, capacity=0)

    def tick(name, t):
        pool, frames = pools[name], {}
        for i, sid in enumerate(sids[name]):
            image, labels, new = srcs[i % 2][t]
            if len(new) > 0:
                torch.manual_seed(0)
                pool.initialize(sid, image, labels, new)
            frames[sid] = image
        out = pool.step(frames)
        if name == 'step+encode' and out:
            index, kept['runs'] = pool.encode(list(out), out=kept.get('runs'))
            seen['ticks'] += 1
            try:
                heads, runs = kept['runs'].cpu()                        # the program sends the lists: they reach the host inside the tick
                seen['most'], seen['capacity'] = max(seen['most'], runs.numel()), kept['runs'].capacity
            except ops.RunsOverflow:
                seen['overflows'] += 1
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
    assert pools['step'].encode_launches == 0 and pools['step+encode'].encode_launches == t - 1
    say('')
    say('## (c) StreamPool, S = %d streams of %d x %d frames, 2 objects each, working size %d x %d' % ((S,) + SRC + WS))
    say('%-14s %-33s %s' % ('arm', 'tick ms (device events)', 're-solve ticks ms'))
    med = {k: statistics.median(ev[k]) for k in arms}
    for k in arms:
        say('%-14s %-33s %s' % (k, fmt(ev[k]), ' '.join('%.3f' % v for v in solve[k])))
    say('# ms: ' + verdict('step', 'step+encode', med, ev))
    say('# %d ticks coded, %d overflowed the default capacity of %d elements; the most run lengths of a tick: %d' % (
        seen['ticks'], seen['overflows'], seen['capacity'], seen['most']))
    for k, p in pools.items():
        for sid in sids[k]:
            p.close(sid)
    del pools
    torch.cuda.empty_cache()


def main():
    prop = torch.cuda.get_device_properties(0)
    say('# Coding the tracked masks of 1080p answers as COCO run lengths on the device; %s (%s, %d CUs); %s' % (
        prop.name, getattr(prop, 'gcnArchName', '?').split(':')[0], prop.multi_processor_count, time.strftime('%Y-%m-%d')))
    say('# (c): ResNet-101, full iteration schedule, memory 80, synthetic sequences, score-following stand-in refiner, working_size=(%d, %d);' % WS)
    say('# timed ticks start after %d warm-up ticks; median [min .. max] of the %d ticks without a filter re-solve.' % (WARM, ROUNDS))
    say("# One arm beats another only when the medians differ by more than the slower arm's own max - min.")
    say('# Not measured: string parity with pycocotools (it is not installed here), and any real decoder, encoder or consumer.')
    params, model = modules()
    srcs = sources(1 + WARM + ROUNDS + ROUNDS // 7 + 3)
    calls(srcs)
    for S in (1, 4, 8):
        pool_ticks(params, model, srcs, S)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


if __name__ == '__main__':
    with torch.no_grad():
        main()
