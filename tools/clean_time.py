"""What cleaning the answer costs: ops.clean_frames (csrc/object_parts.hip) on a 1080 x 1920 answer with 3 objects and about 200 specks,
alone and with its words on the host, against what a caller has without it, and behind StreamPool.step().  Writes profiles/clean_time.txt.
Not part of bench.py.  The method is that of tools/encode_time.py: device events around synchronised work, the arms taking turns in one
process after warm-up, medians with [min .. max] of 16 rounds.

  (a) the call alone: a label map (3 ids) and a K = 3 mask stack, with and without the component map; bytes moved against 6.3 TB/s
  (b) the call plus CleanedAnswers.cpu() -- words and status, one copy --, against the caller's alternative: the device-to-host copy of the
      2 MB label map followed by a connected-component labelling per object on the CPU and the same rule (timed on the host clock: it is
      host work; the copy alone is shown too).  The labelling is scipy.ndimage.label where scipy is installed, else the numpy statement of
      tests/_parts_refs.py; the file says which
  (c) StreamPool ticks of 1, 4 and 8 streams of 1080p frames at working_size=(480, 854): step() alone against step() + clean() with the
      words copied to the host

    python tools/clean_time.py            # everything
    python tools/clean_time.py --calls    # (a) only, a few rounds: the run to put under a kernel trace for the time per phase"""
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
OUT = os.path.join(ROOT, 'profiles', 'clean_time.txt')
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


def speckled(labels, ids, n_specks, seed):
    """``labels`` with ``n_specks`` islands of 1 .. 6 pixels of the objects' ids scattered over it."""
    rng = np.random.default_rng(seed)
    lab = labels.cpu().numpy().copy()
    h, w = lab.shape
    for _ in range(n_specks):
        y, x, oid = int(rng.integers(2, h - 4)), int(rng.integers(2, w - 4)), int(ids[1 + int(rng.integers(0, len(ids) - 1))])
        for dy, dx in [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)][:int(rng.integers(1, 7))]:
            lab[y + dy, x + dx] = oid
    return torch.from_numpy(lab).to(labels.device)


def cpu_labeller():
    try:
        from scipy import ndimage
        structure = np.ones((3, 3), dtype=int)
        return 'scipy.ndimage.label', lambda mask: ndimage.label(mask, structure=structure)[0]
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, 'tests'))
        import _parts_refs
        return 'the numpy statement of tests/_parts_refs.py', lambda mask: _parts_refs.names(np.where(mask, 0, -1), 8) + 1


def cpu_clean(labels, ids, label_parts, min_area):
    """The caller's alternative: the label map to the host, a labelling per object, islands below ``min_area`` set to 0 -> (map, parts per id)."""
    lab = labels.cpu().numpy()
    out, parts = lab.copy(), {}
    for i in ids[1:]:
        comp = label_parts(lab == i)
        area = np.bincount(comp.reshape(-1))
        small = area < min_area
        small[0] = False
        out[small[comp]] = 0
        parts[i] = int((area[1:] > 0).sum())
    return out, parts


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


def calls(srcs, rounds):
    (h, w) = SRC
    labels = srcs[0][0][1]                                              # the first frame: the one that comes with a label map
    labels = (labels if torch.is_tensor(labels) else torch.as_tensor(labels)).to(DEV).reshape(h, w).to(torch.uint8).contiguous()
    ids = sorted(set(labels.unique().tolist()) | {0})[:3]
    while len(ids) < 3:
        ids.append(max(ids) + 1)
    labels = speckled(labels, ids, 200, 7).contiguous()
    lut = torch.tensor(ids, dtype=torch.uint8, device=DEV)
    stack = torch.stack([(labels == i).float() * 0.9 for i in ids]).contiguous()
    rule = dict(connectivity=8, min_area=16)
    kept = {('labels', c): ops.clean_frames([labels], ids=[ids], components=c, **rule) for c in (False, True)}
    kept.update({('stack', c): ops.clean_frames([stack], luts=[lut], components=c, plane_ids=[ids], **rule) for c in (False, True)})
    which, label_parts = cpu_labeller()
    want, want_parts = cpu_clean(labels, ids, label_parts, 16)
    for k, c in kept.items():                                           # the ways state the same map
        assert np.array_equal(c.labels[0].cpu().numpy(), want) and {i: c.objects(0)[i].parts for i in ids[1:]} == want_parts, k
    stats = kept[('labels', False)].objects(0)
    arms = {
        'clean_frames labels (3 ids)': lambda: ops.clean_frames([labels], ids=[ids], out=kept[('labels', False)], **rule),
        'clean_frames labels + components': lambda: ops.clean_frames([labels], ids=[ids], components=True, out=kept[('labels', True)], **rule),
        'clean_frames K=3 stack': lambda: ops.clean_frames([stack], luts=[lut], plane_ids=[ids], out=kept[('stack', False)], **rule),
        'clean_frames K=3 stack + components': lambda: ops.clean_frames([stack], luts=[lut], plane_ids=[ids], components=True, out=kept[('stack', True)], **rule),
        'clean_frames labels + words to host': lambda: ops.clean_frames([labels], ids=[ids], out=kept[('labels', False)], **rule).cpu(),
        'clean_frames K=3 stack + words to host': lambda: ops.clean_frames([stack], luts=[lut], plane_ids=[ids], out=kept[('stack', False)], **rule).cpu(),
    }
    # bytes per pixel: the answer read once (1, or 4 K), then local 1 + 4 + 4 stored, flatten 1 + 4 loaded, slots 1 + 4 loaded, write 1 + 4 + 4
    # loaded and 1 stored (+ 4 with the component map); the seam pass and the stores of flatten touch a small share of the pixels
    nbytes = {name: h * w * ((12 if 'stack' in name else 1) + 29 + (4 if 'components' in name else 0)) for name in arms}
    reps = {name: (10 if 'host' in name else REPS) for name in arms}
    for name, fn in arms.items():                                      # warm-up of every shape
        for _ in range(5):
            fn()
    host_arms = {'label map to host (2 MB copy alone)': lambda: labels.cpu(), 'label map to host + CPU labelling': lambda: cpu_clean(labels, ids, label_parts, 16)}
    for fn in host_arms.values():
        fn()
    ev = {name: [] for name in list(arms) + list(host_arms)}
    for _ in range(rounds):                                             # the arms take turns
        for name, fn in arms.items():
            d, _ = timed(lambda: [fn() for _ in range(reps[name])])
            ev[name].append(d * 1e3 / reps[name])
        for name, fn in host_arms.items():
            d, _ = host_timed(fn)
            ev[name].append(d * 1e3)
    say('')
    say('## (a), (b) one %d x %d answer, 3 objects + 200 specks, connectivity 8, min_area 16: us per call, %d calls back to back between two events' % (SRC + (REPS,)))
    say('## (arms that end on the host: 10; the two "label map to host" arms: one call on the host clock), median [min .. max] of %d rounds, the arms' % rounds)
    say('## taking turns; bytes = what the six kernels load and store (see the source), against %.1f TB/s' % (HBM / 1e12))
    say('%-42s %-36s %10s %10s %8s' % ('call', 'us', 'MB moved', 'us at HBM', 'share'))
    for name in arms:
        bound = nbytes[name] / HBM * 1e6
        say('%-42s %-36s %10.2f %10.2f %7.0f%%' % (name, fmt(ev[name]), nbytes[name] / 1e6, bound, 100 * bound / statistics.median(ev[name])))
    for name in host_arms:
        say('%-42s %-36s' % (name, fmt(ev[name])))
    med = {k: statistics.median(v) for k, v in ev.items()}
    say('# us: ' + verdict('label map to host + CPU labelling', 'clean_frames labels + words to host', med, ev))
    say('# us: ' + verdict('label map to host (2 MB copy alone)', 'clean_frames labels + words to host', med, ev))
    say('# us: ' + verdict('clean_frames labels (3 ids)', 'clean_frames labels + components', med, ev))
    say('# us: ' + verdict('clean_frames labels (3 ids)', 'clean_frames K=3 stack', med, ev))
    say('# the CPU labelling is %s, once per object, on the copied label map, followed by the same min_area rule.' % which)
    say('# a call is ops.clean_frames as a caller makes it on buffers it has cleaned into before: the rows built, their uploaded table found, the')
    say('# size of the workspace asked, SIX enqueued kernels (begin, local, seam, flatten, slots, write).  "+ words to host" adds')
    say('# CleanedAnswers.cpu(): one synchronising copy of 193 words per frame.')
    say('# this answer: ' + '; '.join('id %d: %d parts, %d kept, %d of %d pixels kept' % (i, st.parts, st.kept, st.kept_area, st.area) for i, st in stats.items()))


def pool_ticks(params, model, srcs, S):
    mods = (model.augmenter, model.feature_extractor, params.disc_params, model.refiner, DEV)
    arms = ('step', 'step+clean')
    pools = {k: StreamPool(*mods, max_streams=S, trunk_lanes=params.trunk_lanes, working_size=WS) for k in arms}
    sids = {k: [p.open() for _ in range(S)] for k, p in pools.items()}
    kept = {}
    ev, solve = ({k: [] for k in arms} for _ in range(2))
    seen = dict(ticks=0, most=0)

    def tick(name, t):
        pool, frames = pools[name], {}
        for i, sid in enumerate(sids[name]):
            image, labels, new = srcs[i % 2][t]
            if len(new) > 0:
                torch.manual_seed(0)
                pool.initialize(sid, image, labels, new)
            frames[sid] = image
        out = pool.step(frames)
        if name == 'step+clean' and out:
            index, kept['clean'] = pool.clean(list(out), out=kept.get('clean'), connectivity=8, min_area=16)
            seen['ticks'] += 1
            words, _ = kept['clean'].cpu()                              # the program acts on the numbers: they reach the host inside the tick
            seen['most'] = max(seen['most'], int(words[:, :, 0].sum()))
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
    assert pools['step'].clean_launches == 0 and pools['step+clean'].clean_launches == t - 1
    say('')
    say('## (c) StreamPool, S = %d streams of %d x %d frames, 2 objects each, working size %d x %d' % ((S,) + SRC + WS))
    say('%-14s %-33s %s' % ('arm', 'tick ms (device events)', 're-solve ticks ms'))
    med = {k: statistics.median(ev[k]) for k in arms}
    for k in arms:
        say('%-14s %-33s %s' % (k, fmt(ev[k]), ' '.join('%.3f' % v for v in solve[k])))
    say('# ms: ' + verdict('step', 'step+clean', med, ev))
    say('# %d ticks cleaned; the most parts of a tick, all streams and objects together: %d' % (seen['ticks'], seen['most']))
    for k, p in pools.items():
        for sid in sids[k]:
            p.close(sid)
    del pools
    torch.cuda.empty_cache()


def main():
    calls_only = '--calls' in sys.argv
    prop = torch.cuda.get_device_properties(0)
    say('# Cleaning 1080p answers on the device: connected parts, specks dropped; %s (%s, %d CUs); %s' % (
        prop.name, getattr(prop, 'gcnArchName', '?').split(':')[0], prop.multi_processor_count, time.strftime('%Y-%m-%d')))
    say('# (c): ResNet-101, full iteration schedule, memory 80, synthetic sequences, score-following stand-in refiner, working_size=(%d, %d);' % WS)
    say('# timed ticks start after %d warm-up ticks; median [min .. max] of the %d ticks without a filter re-solve.' % (WARM, ROUNDS))
    say("# One arm beats another only when the medians differ by more than the slower arm's own max - min.")
    say('# The pictures are synthetic: no real tracker answers with real distractors were available.')
    srcs = sources(2 if calls_only else 1 + WARM + ROUNDS + ROUNDS // 7 + 3)
    calls(srcs, 2 if calls_only else ROUNDS)
    if calls_only:
        return
    params, model = modules()
    for S in (1, 4, 8):
        pool_ticks(params, model, srcs, S)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


if __name__ == '__main__':
    with torch.no_grad():
        main()
