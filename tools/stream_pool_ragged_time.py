"""What one refiner pass for streams with DIFFERENT object counts buys a StreamPool tick: ``ragged_groups`` off against on, 480x854,
ResNet-101, the full iteration schedule, synthetic sequences, one frame per stream and tick.  Writes profiles/stream_pool_ragged_time.txt.
Not part of bench.py.  The method is that of tools/stream_pool_time.py.

Four arms take turns in one process after warm-up, each a StreamPool with target models of its own on the same frames:
  off     ragged_groups=False, grouped_apply=False: one refiner pass, one merge per distinct object count (plan_tick)
  on      ragged_groups=True,  grouped_apply=False: one refiner pass and one merge per tick (plan_tick_ragged, csrc/ragged_group.hip)
  off+g   ragged_groups=False, grouped_apply=True (min_pairs=1): plus one grouped scoring launch per distinct object count
  on+g    ragged_groups=True,  grouped_apply=True (min_pairs=1): plus ONE grouped scoring launch per tick
on S = 8 streams with 1, 1, 2, 2, 3, 3, 4 and 5 objects, on S = 4 with 1, 2, 3 and 4, and -- the control -- on S = 8 with 2 objects each,
where both planners plan the same launches.  A tick is timed from the device: synchronise, event, the arm's tick, event.  The streams run
in lock step, so every 8th tick re-solves every filter: those ticks are listed on their own, the table's 24 rounds are the ticks without
a re-solve.

    python tools/stream_pool_ragged_time.py"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd.evaluate import Parameters  # noqa: E402
from frtm_vos_amd.lib.synthetic import SyntheticSequence, make_score_following_refiner  # noqa: E402
from frtm_vos_amd.model.seg_network import SegNetwork  # noqa: E402
from frtm_vos_amd.model.stream_pool import StreamPool  # noqa: E402

DEV = 'cuda:0'
OUT = os.path.join(ROOT, 'profiles', 'stream_pool_ragged_time.txt')
HW = (480, 854)
ROUNDS = 24
WARM = 9                       # ticks before the first timed one: past the first filter re-solve (frame 8)
CONFIGS = (('S = 8, 1 1 2 2 3 3 4 5 objects', (1, 1, 2, 2, 3, 3, 4, 5)), ('S = 4, 1 2 3 4 objects', (1, 2, 3, 4)),
           ('control: S = 8, 2 objects each', (2,) * 8))
ARMS = (('off', False, False), ('on', False, True), ('off+g', True, False), ('on+g', True, True))      # (name, grouped_apply, ragged_groups)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def fmt(v):
    return '%7.3f [%7.3f .. %7.3f]' % (statistics.median(v), min(v), max(v))


def modules():
    """One augmenter, trunk and refiner for every arm (the refiner: the score-following stand-in for a trained one, as bench.py)."""
    def refiner(chans):
        torch.manual_seed(1)
        return make_score_following_refiner(SegNetwork(1, 64, chans, True).eval())
    params = Parameters(None, fast=False, device=DEV, feature_extractor='resnet101')
    params.refiner_factory = refiner
    return params, params.get_model().eval()


class Arms:
    """The four pools over one set of streams; ``tick(name, t)`` runs frame t of every stream through one of them."""

    def __init__(self, params, model, seqs):
        self.seqs = seqs
        mods = (model.augmenter, model.feature_extractor, params.disc_params, model.refiner, DEV)
        self.pools = {name: StreamPool(*mods, max_streams=len(seqs), grouped_apply=grouped, min_pairs=1, trunk_lanes=params.trunk_lanes,
                                       ragged_groups=ragged) for name, grouped, ragged in ARMS}
        self.sids = {k: [p.open() for _ in seqs] for k, p in self.pools.items()}

    def tick(self, name, t):
        pool, frames = self.pools[name], {}
        for sid, seq in zip(self.sids[name], self.seqs):
            image, labels, new_objects = seq[t]
            if len(new_objects) > 0:
                pool.initialize(sid, image, labels, new_objects)
            frames[sid] = image
        pool.step(frames)

    def close(self):
        for k, p in self.pools.items():
            for sid in self.sids[k]:
                p.close(sid)


def timed_tick(arms, name, t):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    w0 = time.perf_counter()
    e0.record()
    arms.tick(name, t)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - w0) * 1e3


def verdict(a, b, med, ev):
    """``b`` against ``a`` by the rule of the bf16x1 routers."""
    d, spread = med[b] - med[a], max(ev[a]) - min(ev[a])
    word = 'FASTER' if -d > spread else ('inside the spread' if abs(d) <= spread else 'SLOWER')
    return '%s - %s = %+.3f ms against a spread of %.3f ms in %s: %s' % (b, a, d, spread, a, word)


def measure(params, model, title, counts, n_frames):
    seqs = [SyntheticSequence('r%d' % k, n_frames, HW, n, seed=100 + k) for k, n in enumerate(counts)]
    for s in seqs:
        s.preload(DEV)
    arms = Arms(params, model, seqs)
    names = [a[0] for a in ARMS]
    ev, wall, solve = ({k: [] for k in names} for _ in range(3))
    plan = {}
    t = 0
    while len(ev[names[0]]) < ROUNDS:
        for name in (names if t % 2 == 0 else names[::-1]):
            if t <= WARM:
                arms.tick(name, t)
                continue
            pool = arms.pools[name]
            before = (pool.refiner_passes, pool.grouped_launches)
            d, w = timed_tick(arms, name, t)
            plan.setdefault(name, set()).add((pool.refiner_passes - before[0], pool.grouped_launches - before[1]))
            if t % 8 == 0:
                solve[name].append(d)
            else:
                ev[name].append(d)
                wall[name].append(w)
        t += 1
    arms.close()
    S, pairs = len(counts), sum(counts)
    say('')
    say('## %s (%d pairs)' % (title, pairs))
    say('%-6s %-22s %-29s %-29s %12s' % ('arm', 'refiner passes / grouped', 'tick ms (device events)', 'tick ms (host wall clock)', 'ms per frame'))
    med = {k: statistics.median(ev[k]) for k in names}
    for k in names:
        launches = ' or '.join('%d / %d' % p for p in sorted(plan[k]))
        say('%-6s %-22s   %-29s %-29s %12.3f' % (k, launches, fmt(ev[k]), fmt(wall[k]), med[k] / S))
    say('       re-solve ticks (ms): ' + '   '.join('%s %s' % (k, ' '.join('%.3f' % v for v in solve[k])) for k in names))
    say('# ' + verdict('off', 'on', med, ev))
    say('# ' + verdict('off+g', 'on+g', med, ev))
    if len(set(counts)) == 1:
        same = plan['off'] == plan['on'] and plan['off+g'] == plan['on+g']
        say('# control: both planners plan %s launches per tick' % ('the SAME' if same else 'DIFFERENT'))
    del arms, seqs
    torch.cuda.empty_cache()


def main():
    prop = torch.cuda.get_device_properties(0)
    say('# StreamPool ticks with ragged_groups off and on; %s (%s, %d CUs); %s' % (
        prop.name, getattr(prop, 'gcnArchName', '?').split(':')[0], prop.multi_processor_count, time.strftime('%Y-%m-%d')))
    say('# 480x854, ResNet-101, full iteration schedule, memory 80, synthetic sequences; one frame per stream and tick.')
    say('# off / on = StreamPool(ragged_groups=False / True); +g = grouped_apply=True, min_pairs=1.  "refiner passes / grouped": refiner calls and')
    say('# grouped scoring launches per timed tick.  Arms alternate in one process after %d warm-up ticks; median [min .. max] of the %d ticks' % (WARM, ROUNDS))
    say("# without a filter re-solve.  Rule of the bf16x1 routers: one arm beats another when the medians differ by more than the other arm's max - min.")
    params, model = modules()
    n_frames = 1 + WARM + ROUNDS + ROUNDS // 7 + 3
    for title, counts in CONFIGS:
        measure(params, model, title, counts, n_frames)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


if __name__ == '__main__':
    with torch.no_grad():
        main()
