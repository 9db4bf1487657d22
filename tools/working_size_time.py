"""What tracking at a working size costs and buys: Tracker / StreamPool with ``working_size=(480, 854)`` against frames tracked at the
size they arrive in.  ResNet-101, the full iteration schedule, synthetic sequences, the score-following stand-in for a trained refiner
(as bench.py).  Writes profiles/working_size_time.txt.  Not part of bench.py.  The method is that of tools/stream_pool_time.py: device
events around synchronised work, the arms taking turns in one process after warm-up, medians with [min .. max].

  (a) per-frame track(): 2 objects on 1080 x 1920 and 720 x 1280 frames, native against the working size (resize in, step, masks out)
  (b) StreamPool: four streams of four different frame sizes, 2 objects each, without and with the working size: ms per tick, trunk passes
  (c) the kernels alone: masks_to_native, resize_label_map_u8 and the inbound resize_frames_u8, against their byte counts at 6.3 TB/s
  (d) J&F on synthetic sequences rendered at 720 x 1280, native against the working size, one run each

    python tools/working_size_time.py"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd import ops  # noqa: E402
from frtm_vos_amd.evaluate import Parameters  # noqa: E402
from frtm_vos_amd.lib.evaluation import j_and_f  # noqa: E402
from frtm_vos_amd.lib.synthetic import SyntheticSequence, make_score_following_refiner  # noqa: E402
from frtm_vos_amd.model.seg_network import SegNetwork  # noqa: E402
from frtm_vos_amd.model.stream_pool import StreamPool  # noqa: E402
from frtm_vos_amd.model.tracker import Tracker  # noqa: E402

DEV = 'cuda:0'
OUT = os.path.join(ROOT, 'profiles', 'working_size_time.txt')
WS = (480, 854)
ROUNDS = 16
WARM = 9                       # frames before the first timed one: past the first filter re-solve (frame 8)
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


def modules():
    def refiner(chans):
        torch.manual_seed(1)
        return make_score_following_refiner(SegNetwork(1, 64, chans, True).eval())
    params = Parameters(None, fast=False, device=DEV, feature_extractor='resnet101')
    params.refiner_factory = refiner
    return params, params.get_model().eval()


def tracker(params, model, working_size):
    return Tracker(model.augmenter, model.feature_extractor, params.disc_params, model.refiner, DEV, working_size=working_size).eval()


def verdict(a, b, med, ev):
    d, spread = med[b] - med[a], max(ev[a]) - min(ev[a])
    word = 'FASTER' if -d > spread else ('inside the spread' if abs(d) <= spread else 'SLOWER')
    return '%s - %s = %+.3f ms against a spread of %.3f ms in %s: %s' % (b, a, d, spread, a, word)


def per_frame(params, model, size):
    seq = SyntheticSequence('f', 1 + WARM + ROUNDS + ROUNDS // 7 + 3, size, 2, seed=41)
    seq.preload(DEV)
    arms = {'native': tracker(params, model, None), 'working': tracker(params, model, WS)}
    ev, solve, init = ({k: [] for k in arms} for _ in range(3))
    t = 0
    while len(ev['native']) < ROUNDS:
        image, labels, new = seq[t]
        for name in (list(arms) if t % 2 == 0 else list(arms)[::-1]):
            trk = arms[name]
            if len(new) > 0:
                torch.manual_seed(0)
                init[name].append(timed(lambda: trk.initialize(image, labels, new))[0])
            else:
                d = timed(lambda: trk.track(image))[0]
                if t > WARM:
                    (solve if t % 8 == 0 else ev)[name].append(d)
            trk.current_frame += 1
        t += 1
    say('')
    say('## (a) track() per frame, %d x %d frames, 2 objects' % size)
    say('%-8s %-33s %-14s %s' % ('arm', 'track() ms (device events)', 'initialize ms', 're-solve frames ms'))
    med = {k: statistics.median(ev[k]) for k in arms}
    for k in arms:
        say('%-8s %-33s %-14.1f %s' % (k, fmt(ev[k]), init[k][0], ' '.join('%.3f' % v for v in solve[k])))
    say('# ' + verdict('native', 'working', med, ev) + '; native / working = %.2fx' % (med['native'] / med['working']))
    for trk in arms.values():
        trk.release_targets()
    del arms, seq
    torch.cuda.empty_cache()


def pool_ticks(params, model):
    sizes = ((480, 854), (720, 1280), (1080, 1920), (360, 640))
    seqs = [SyntheticSequence('p%d' % k, 1 + WARM + ROUNDS + ROUNDS // 7 + 3, s, 2, seed=60 + k) for k, s in enumerate(sizes)]
    for s in seqs:
        s.preload(DEV)
    mods = (model.augmenter, model.feature_extractor, params.disc_params, model.refiner, DEV)
    pools = {'native': StreamPool(*mods, max_streams=4, trunk_lanes=params.trunk_lanes),
             'working': StreamPool(*mods, max_streams=4, trunk_lanes=params.trunk_lanes, working_size=WS)}
    sids = {k: [p.open() for _ in seqs] for k, p in pools.items()}
    ev, solve, passes = ({k: [] for k in pools} for _ in range(3))

    def tick(name, t):
        pool, frames = pools[name], {}
        for sid, seq in zip(sids[name], seqs):
            image, labels, new = seq[t]
            if len(new) > 0:
                torch.manual_seed(0)
                pool.initialize(sid, image, labels, new)
            frames[sid] = image
        return pool.step(frames)
    t = 0
    while len(ev['native']) < ROUNDS:
        for name in (list(pools) if t % 2 == 0 else list(pools)[::-1]):
            if t <= WARM:
                tick(name, t)
                continue
            before = pools[name].trunk_passes
            d, out = timed(lambda: tick(name, t))
            assert all(tuple(out[sid].shape[-2:]) == s for sid, s in zip(sids[name], sizes))      # native-size masks in both arms
            passes[name].append(pools[name].trunk_passes - before)
            (solve if t % 8 == 0 else ev)[name].append(d)
        t += 1
    say('')
    say('## (b) StreamPool, four streams at %s, 2 objects each' % ', '.join('%d x %d' % s for s in sizes))
    say('%-8s %-14s %-33s %s' % ('arm', 'trunk passes', 'tick ms (device events)', 're-solve ticks ms'))
    med = {k: statistics.median(ev[k]) for k in pools}
    for k in pools:
        say('%-8s %-14s %-33s %s' % (k, ' or '.join(str(p) for p in sorted(set(passes[k]))), fmt(ev[k]), ' '.join('%.3f' % v for v in solve[k])))
    say('# ' + verdict('native', 'working', med, ev) + '; native / working = %.2fx' % (med['native'] / med['working']))
    for k, p in pools.items():
        for sid in sids[k]:
            p.close(sid)
    del pools, seqs
    torch.cuda.empty_cache()


def kernel_us(fn, reps=50):
    for _ in range(5):
        fn()
    samples = []
    for _ in range(7):
        d, _ = timed(lambda: [fn() for _ in range(reps)])
        samples.append(d * 1e3 / reps)
    return samples


def kernels():
    say('')
    say('## (c) the kernels alone: us per launch, %d launches back to back between two events, median [min .. max] of 7; bytes / %.1f TB/s' % (50, HBM / 1e12))
    say('%-64s %-33s %10s %10s %8s' % ('launch', 'us', 'MB moved', 'us at HBM', 'share'))
    h, w = WS
    g = torch.Generator().manual_seed(0)

    def row(name, samples, nbytes):
        bound = nbytes / HBM * 1e6
        say('%-64s %-33s %10.2f %10.2f %7.0f%%' % (name, fmt(samples), nbytes / 1e6, bound, 100 * bound / statistics.median(samples)))
    for K, natives in ((3, [(1080, 1920)]), (3, [(720, 1280)]), (3, [(480, 854), (720, 1280), (1080, 1920), (360, 640)])):
        masks = torch.rand(len(natives), K, h, w, generator=g).to(DEV)
        lut = torch.arange(K, dtype=torch.uint8, device=DEV)
        for soft in (False, True):
            table = ops.NativeTable.packed(WS, [(K,) + n for n in natives], DEV, soft=soft, shared_lut=True)
            labels = torch.empty(table.label_bytes, dtype=torch.uint8, device=DEV)
            planes = torch.empty(table.soft_elems, device=DEV) if soft else None
            nbytes = sum(K * h * w * 4 + Hn * Wn + (K * Hn * Wn * 4 if soft else 0) for Hn, Wn in natives)
            row('masks_to_native K = %d, 480 x 854 -> %s, %s' % (K, ' + '.join('%dx%d' % n for n in natives), 'labels + soft planes' if soft else 'labels'),
                kernel_us(lambda: ops.masks_to_native(masks, table, labels, lut, soft=planes)), nbytes)
    for Hn, Wn in ((1080, 1920), (720, 1280)):
        lab = torch.randint(0, 3, (Hn * Wn,), generator=g, dtype=torch.uint8).to(DEV)
        plan = ops.ResizePlan(torch.tensor([[0, Hn, Wn, 0]]), DEV)
        out = torch.empty(1, 1, h, w, dtype=torch.uint8, device=DEV)
        row('resize_label_map_u8 %d x %d -> 480 x 854 (bytes: the source rows it touches + out)' % (Hn, Wn),
            kernel_us(lambda: plan.label_map(lab, WS, out=out)), h * Wn + h * w)
        frame = torch.randint(0, 256, (3 * Hn * Wn,), generator=g, dtype=torch.uint8).to(DEV)
        fplan = ops.ResizePlan(torch.tensor([[0, Hn, Wn, ops.RESIZE_MODES['area']]]), DEV)
        fout = torch.empty(1, 3, h, w, dtype=torch.uint8, device=DEV)
        row("resize_frames_u8 'area' 3 x %d x %d -> 480 x 854 (inbound)" % (Hn, Wn), kernel_us(lambda: fplan.frames(frame, 3, WS, out=fout)), 3 * Hn * Wn + 3 * h * w)
    say('# a launch of a few us is bound by launch latency, not by bytes: the share column says how far from the byte bound a launch is, nothing more.')


def accuracy(params, model):
    size = (720, 1280)
    seqs = [SyntheticSequence('j%d' % k, 20, size, n, seed=80 + k) for k, n in enumerate((1, 2, 2, 3))]
    res = {}
    for name, ws in (('native', None), ('working', WS)):
        trk = tracker(params, model, ws)
        vals = []
        for seq in seqs:
            seq.preload(DEV)
            torch.manual_seed(0)
            out, _ = trk.run_sequence(seq)
            pred = torch.stack([o.reshape(size) for o in out])
            gt = torch.stack([g_.reshape(size).to(DEV) for g_ in seq.gt])
            vals.append(j_and_f(pred, gt, seq.obj_ids))
            seq.release()
        res[name] = [sum(v[i] for v in vals) / len(vals) for i in range(3)]
        trk.release_targets()
    say('')
    say('## (d) J&F, %d synthetic sequences of 20 frames rendered at %d x %d (1, 2, 2, 3 objects), run_sequence, one run each' % (len(seqs), size[0], size[1]))
    for k, (jf, j, f) in res.items():
        say('%-8s J&F %.3f   J %.3f   F %.3f' % (k, jf, j, f))
    say('# working - native: J&F %+.3f.  Synthetic rectangles and a stand-in refiner: this says that the way in and back works, not what a trained' % (res['working'][0] - res['native'][0]))
    say("# model loses; the README's single-run sigma of dataset-level J&F (fixture G14) is 0.064-0.067.")


def main():
    prop = torch.cuda.get_device_properties(0)
    say('# Tracking at a working size of %d x %d against native size; %s (%s, %d CUs); %s' % (
        WS + (prop.name, getattr(prop, 'gcnArchName', '?').split(':')[0], prop.multi_processor_count, time.strftime('%Y-%m-%d'))))
    say('# ResNet-101, full iteration schedule, memory 80, synthetic sequences, score-following stand-in refiner.  native = working_size=None (the')
    say('# behaviour without the option); working = working_size=(%d, %d).  Arms alternate in one process; timed frames start after %d warm-up' % (WS + (WARM,)))
    say("# frames; median [min .. max] of the %d frames without a filter re-solve.  One arm beats another when the medians differ by more than the other arm's max - min." % ROUNDS)
    params, model = modules()
    for size in ((1080, 1920), (720, 1280)):
        per_frame(params, model, size)
    pool_ticks(params, model)
    kernels()
    accuracy(params, model)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


if __name__ == '__main__':
    with torch.no_grad():
        main()
