"""What batching ACROSS live streams buys: S streams of one frame per tick, 480x854, ResNet-101, 2 objects per stream, the full iteration
schedule, synthetic sequences.  Writes profiles/stream_pool_time.txt.  Not part of bench.py.

Three arms take turns in one process after warm-up, each with target models of its own on the same frames:
  (A) S independent Trackers, each stepping track(image) once per tick -- all the project offered a live application before StreamPool;
  (B) StreamPool(grouped_apply=False): one trunk pass, one refiner pass and one merge per tick, target models scored pair by pair;
  (C) StreamPool(grouped_apply=True): the same with ONE ops.target_apply_grouped launch pair for all pairs.
A tick is timed from the device: synchronise, event, the arm's tick, event.  The streams run in lock step, so every 8th tick re-solves
every filter: those ticks are listed on their own, the table's 24 rounds are the ticks without a re-solve.

    python tools/stream_pool_time.py                     the tables (S = 1, 2, 4, 8, 16; then TrainerModel.forward at B = 16)
    python tools/stream_pool_time.py --kernels-only      the scoring step of a tick at S = 8 both ways and nothing else: the run to put under
                                                         rocprofv3 --kernel-trace --stats
    python tools/stream_pool_time.py --stats-csv FILE    append the scoring kernels' times from that run's kernel_trace.csv"""
import csv
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd.evaluate import Parameters  # noqa: E402
from frtm_vos_amd.lib.synthetic import SyntheticSequence, make_score_following_refiner  # noqa: E402
from frtm_vos_amd.model.seg_network import SegNetwork  # noqa: E402
from frtm_vos_amd.model.stream_pool import StreamPool  # noqa: E402
from frtm_vos_amd.model.tracker import Tracker  # noqa: E402

DEV = 'cuda:0'
OUT = os.path.join(ROOT, 'profiles', 'stream_pool_time.txt')
HW = (480, 854)
N_OBJ = 2
ROUNDS = 24
WARM = 9                       # ticks before the first timed one: past the first filter re-solve (frame 8)
SIZES = (1, 2, 4, 8, 16)
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
    """The three arms over S streams; ``tick(name, t)`` runs frame t of every stream through one arm."""

    def __init__(self, params, model, seqs):
        self.seqs = seqs
        S = len(seqs)
        mods = (model.augmenter, model.feature_extractor, params.disc_params, model.refiner, DEV)
        self.trackers = [Tracker(*mods).eval() for _ in range(S)]
        self.pools = {'B': StreamPool(*mods, max_streams=S, grouped_apply=False, trunk_lanes=params.trunk_lanes),
                      'C': StreamPool(*mods, max_streams=S, grouped_apply=True, min_pairs=1, trunk_lanes=params.trunk_lanes)}
        self.sids = {k: [p.open() for _ in range(S)] for k, p in self.pools.items()}

    def tick(self, name, t):
        if name == 'A':
            for trk, seq in zip(self.trackers, self.seqs):
                image, labels, new_objects = seq[t]
                had = len(trk.targets) > 0
                if len(new_objects) > 0:
                    trk.initialize(image, labels, new_objects)
                if had:
                    trk.track(image)
                trk.current_frame += 1
            return
        pool, sids = self.pools[name], self.sids[name]
        frames = {}
        for sid, seq in zip(sids, self.seqs):
            image, labels, new_objects = seq[t]
            if len(new_objects) > 0:
                pool.initialize(sid, image, labels, new_objects)
            frames[sid] = image
        pool.step(frames)

    def close(self):
        for trk in self.trackers:
            trk.release_targets()
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


def sweep(params, model, all_seqs):
    say('%-3s %-5s %-3s %-29s %-29s %10s %12s' % ('S', 'pairs', 'arm', 'tick ms (device events)', 'tick ms (host wall clock)', 'frames/s', 'ms per frame'))
    verdict = []
    for S in SIZES:
        arms = Arms(params, model, all_seqs[:S])
        ev = {k: [] for k in 'ABC'}
        wall = {k: [] for k in 'ABC'}
        solve = {k: [] for k in 'ABC'}
        t = 0
        while len(ev['A']) < ROUNDS:
            order = ('A', 'B', 'C') if t % 2 == 0 else ('C', 'B', 'A')
            for name in order:
                if t <= WARM:
                    arms.tick(name, t)
                    continue
                d, w = timed_tick(arms, name, t)
                if t % 8 == 0:
                    solve[name].append(d)
                else:
                    ev[name].append(d)
                    wall[name].append(w)
            t += 1
        arms.close()
        med = {k: statistics.median(ev[k]) for k in 'ABC'}
        for k in 'ABC':
            say('%-3d %-5d %-3s %-29s %-29s %10.1f %12.3f' % (S, S * N_OBJ, k, fmt(ev[k]), fmt(wall[k]), 1e3 * S / med[k], med[k] / S))
        say('        re-solve ticks (ms): ' + '   '.join('%s %s' % (k, ' '.join('%.3f' % v for v in solve[k])) for k in 'ABC'))
        spread_b, spread_a = max(ev['B']) - min(ev['B']), max(ev['A']) - min(ev['A'])
        verdict.append((S, med, spread_a, spread_b))
        torch.cuda.empty_cache()
    say('')
    say("# rule of the bf16x1 routers: one arm beats another when the medians differ by more than the slower arm's own max - min")
    first = None
    for S, med, spread_a, spread_b in verdict:
        c_b = med['B'] - med['C'] > spread_b
        say('# S = %2d (%2d pairs): C - B = %+.3f ms against a B spread of %.3f ms: grouped scoring %s;   pool (C) - A = %+.3f ms against an A spread of %.3f ms: the pool %s' % (
            S, S * N_OBJ, med['C'] - med['B'], spread_b, 'FASTER' if c_b else ('inside the spread' if abs(med['C'] - med['B']) <= spread_b else 'SLOWER'),
            med['C'] - med['A'], spread_a, 'FASTER' if med['A'] - med['C'] > spread_a else ('inside the spread' if abs(med['C'] - med['A']) <= spread_a else 'SLOWER')))
        if c_b and first is None:
            first = S * N_OBJ
    say('# min_pairs by that rule: %s' % (first if first is not None else 'none measured -- grouped_apply should default to False'))


def trainer_forward():
    """TrainerModel.forward at B = 16 with and without batched_scores (target models from the cache after the first call)."""
    from frtm_vos_amd.model.augmenter import ImageAugmenter
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    from frtm_vos_amd.model.training_model import SampleSpec, TrainerModel
    B = 16
    P = Parameters(None, fast=False, device=DEV, feature_extractor='resnet101')
    P.disc_params.update(c_channels=32, memory_size=20, pixel_weighting=None)
    ext = ResnetFeatureExtractor('resnet101').to(DEV)
    chans = {L: n for L, n in ext.get_out_channels().items() if L in P.refnet_params.layers}
    torch.manual_seed(1)
    net = SegNetwork(1, 64, chans, True).to(DEV)
    seqs = [SyntheticSequence('t%d' % k, 3, HW, 1, seed=50 + k) for k in range(B)]
    images = [torch.stack([s.images[t] for s in seqs]).to(DEV) for t in range(3)]
    labels = [torch.stack([(s.gt[t] == 1).to(torch.uint8) for s in seqs]).to(DEV) for t in range(3)]
    meta = [SampleSpec('t%d' % k, 1, [0, 1, 2], 0).encoded() for k in range(B)]
    cache = dict(path=tempfile.mkdtemp(prefix='tmcache'), enable=True, read_only=False)
    arms = {}
    for name, batched in (('per sample', False), ('per sample (2nd instance)', False), ('--batched-scores', True)):
        arms[name] = TrainerModel(ImageAugmenter(P.aug_params), ext, P.disc_params, net, batch_size=B, tmodel_cache=cache, device=DEV,
                                  refiner_backend='hip', loss_backend='hip', batched_scores=batched)
    t = {k: [] for k in arms}
    with torch.enable_grad():
        for r in range(2 + 8):
            for name, m in arms.items():
                net.zero_grad()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m(images, labels, meta)
                e1.record()
                e1.synchronize()
                if r >= 2:
                    t[name].append(e0.elapsed_time(e1))
    say('')
    say('# TrainerModel.forward, B = 16, ResNet-101, 480x854, 3 frames per sample, c = 32, target models read from the cache; 8 repetitions after 2 warm-up')
    for name, v in t.items():
        say('%-28s %s ms' % (name, fmt(v)))


def kernels_only():
    """Nothing but the scoring step of a tick at S = 8 (16 pairs on 8 frames of 1024 x 30 x 54 features), 20 times each way: every kernel
    of the trace that is not one of the two grouped ones belongs to the per-pair path."""
    from frtm_vos_amd import ops
    from frtm_vos_amd.model.discriminator import Discriminator
    params = Parameters(None, fast=False, device=DEV, feature_extractor='resnet101')
    S, P = 8, 8 * N_OBJ
    discs = [Discriminator(**params.disc_params) for _ in range(P)]
    c = discs[0].project.out_channels
    ft = torch.randn(S, 1024, 30, 54, device=DEV).relu()
    scores = torch.empty(P, 1, 30, 54, device=DEV)
    cft = torch.empty(P, c, 30, 54, device=DEV)
    w1T = ops.pointer_table([d._project_T() for d in discs], DEV)
    w2 = ops.pointer_table([d.filter.weight.data for d in discs], DEV)
    frames = (torch.arange(P, dtype=torch.int32) // N_OBJ).to(DEV)
    for _ in range(20):
        for p, d in enumerate(discs):
            d.apply(ft[p // N_OBJ:p // N_OBJ + 1], interleave=(scores, p, P))
        ops.target_apply_grouped(ft, frames, w1T, w2, c, cft=cft, scores=scores)
    torch.cuda.synchronize()


def append_stats(path):
    """Rows of that run's kernel_trace.csv, per kernel and grid."""
    groups = {}
    for r in csv.DictReader(open(path)):
        k = r.get('Kernel_Name', '')
        short = k.split('(')[0].replace('void ', '')
        if 'k_transpose2d' in k or 'randn' in k or 'distribution' in k or 'elementwise' in k:
            continue                                                     # (set-up: the GEMM-layout copies of the projections, the random features)
        key = ('grouped   ' if 'k_grouped' in k else 'per pair  ') + short[:70] + ' grid %sx%sx%s' % (
            r.get('Grid_Size_X', '?'), r.get('Grid_Size_Y', '?'), r.get('Grid_Size_Z', '?'))
        groups.setdefault(key, []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    with open(OUT, 'a') as f:
        f.write('\n# per kernel, from a separate `rocprofv3 --kernel-trace --stats -- python tools/stream_pool_time.py --kernels-only` run: the scoring\n'
                '# step of one tick at S = 8 (16 pairs, 1024 x 30 x 54 features) 20 times each way; grid in work-items; "sum" = calls x median / 20 = per tick\n')
        f.write('%-112s %6s %10s %10s %10s %10s\n' % ('kernel', 'calls', 'median us', 'min us', 'max us', 'sum us'))
        for name, ns in sorted(groups.items()):
            med = statistics.median(ns) / 1e3
            f.write('%-112s %6d %10.2f %10.2f %10.2f %10.2f\n' % (name, len(ns), med, min(ns) / 1e3, max(ns) / 1e3, med * len(ns) / 20))
    print('appended %d rows to %s' % (len(groups), OUT))


def main():
    prop = torch.cuda.get_device_properties(0)
    say('# StreamPool against S independent track(image) loops; %s (%s, %d CUs); %s' % (
        prop.name, getattr(prop, 'gcnArchName', '?').split(':')[0], prop.multi_processor_count, time.strftime('%Y-%m-%d')))
    say('# 480x854, ResNet-101, %d objects per stream, full iteration schedule, memory 80, synthetic sequences; one frame per stream and tick.' % N_OBJ)
    say('# A = S Trackers stepping track(image); B = StreamPool(grouped_apply=False); C = StreamPool(grouped_apply=True, min_pairs=1).')
    say('# Arms alternate in one process after %d warm-up ticks; median [min .. max] of the %d ticks without a filter re-solve.' % (WARM, ROUNDS))
    params, model = modules()
    n_frames = 1 + WARM + ROUNDS + ROUNDS // 7 + 3
    all_seqs = [SyntheticSequence('p%d' % k, n_frames, HW, N_OBJ, seed=100 + k) for k in range(max(SIZES))]
    for s in all_seqs:
        s.preload(DEV)
    sweep(params, model, all_seqs)
    del params, model, all_seqs
    torch.cuda.empty_cache()
    trainer_forward()
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


if __name__ == '__main__':
    if '--kernels-only' in sys.argv:
        kernels_only()
    elif '--stats-csv' in sys.argv:
        append_stats(sys.argv[sys.argv.index('--stats-csv') + 1])
    else:
        with torch.no_grad():
            main()
