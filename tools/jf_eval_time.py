"""Time of J&F scoring on the GPU (lib/evaluation.py: j_and_f on device label maps -> csrc/jf_eval.hip) against the numpy path on the same
maps, and against the time to track the sequence.  Writes profiles/jf_eval_time.txt.

Both arms run in one process, alternating, after a warm-up call per shape; the host clock runs around whole calls, which end in the
device-to-host read of the counts (GPU arm) or start from host arrays (numpy arm).
    python tools/jf_eval_time.py                      the table
    python tools/jf_eval_time.py --score-only         a few GPU scoring calls and nothing else: the run to put under
                                                      rocprofv3 --kernel-trace --stats
    python tools/jf_eval_time.py --stats-csv FILE     append the k_jf_* launches of that run's kernel_trace.csv to the profile, by launch shape"""
import copy
import csv
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd.lib.evaluation import j_and_f  # noqa: E402
from frtm_vos_amd.lib.synthetic import SyntheticSequence  # noqa: E402

DEV = 'cuda:0'
OUT = os.path.join(ROOT, 'profiles', 'jf_eval_time.txt')
ROUNDS = 7
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def shifted(gt, dy=2, dx=-3):
    """Predictions for a shape no tracker runs on here: the ground truth moved by (dy, dx) pixels."""
    return [torch.roll(g, (dy, dx), (-2, -1)) for g in gt]


def tracker_and_labels(seq):
    """The headline tracker (ResNet-101, two objects) on `seq`: its label maps (device tensors) and the median seconds of a run."""
    import oracle.make_golden_jf as JF
    from oracle.tracker_ref import shift_flip_augment
    from frtm_vos_amd.evaluate import Parameters
    params = Parameters(None, device=DEV, feature_extractor='resnet101')
    refiner = JF.refiner_for('resnet101')
    params.refiner_factory = lambda chans, r=refiner: copy.deepcopy(r)
    params.disc_params.update(**JF.DISC)
    trk = params.get_model().eval()
    trk.augment = shift_flip_augment
    trk.start_weights = lambda oid: JF.start_weights(7, oid)
    trk.run_sequence(seq)                                       # warm-up
    secs, labels = [], None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        labels, _ = trk.run_sequence(seq)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    return labels, statistics.median(secs)


def time_shape(name, pred_d, gt_d, ids):
    """Alternating rounds of the two arms on the same maps; returns (median ms GPU, median ms numpy)."""
    size = tuple(gt_d[0].shape[-2:])
    pred_h = [p.reshape(size).cpu().numpy() for p in pred_d]
    gt_h = [g.reshape(size).cpu().numpy() for g in gt_d]
    a, b = j_and_f(pred_d, gt_d, ids), j_and_f(pred_h, gt_h, ids)              # warm-up of both arms; the values must agree exactly
    assert a == b, (a, b)
    tg, tn = [], []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        j_and_f(pred_d, gt_d, ids)                                              # ends in the device-to-host read of the counts
        t1 = time.perf_counter()
        j_and_f(pred_h, gt_h, ids)
        t2 = time.perf_counter()
        tg.append((t1 - t0) * 1e3)
        tn.append((t2 - t1) * 1e3)
    g, n = statistics.median(tg), statistics.median(tn)
    say('%-44s  J&F %.3f  GPU %8.3f ms (min %.3f)  numpy %9.1f ms  ratio %6.0fx' % (name, float(a[0]), g, min(tg), n, n / g))
    return g, n


def sequences():
    seq = SyntheticSequence('jf480', 20, (480, 854), 2, seed=7)
    seq.preload(DEV)
    big = SyntheticSequence('jf1080', 8, (1080, 1920), 8, seed=9)
    big.preload(DEV)
    return seq, big


def score_only():
    seq, big = sequences()
    for s in (seq, big):
        pred = shifted(s.gt)
        for _ in range(3):
            j_and_f(pred, s.gt, s.obj_ids)
    torch.cuda.synchronize()


def append_stats(path):
    """Per-kernel times by launch shape from rocprofv3's kernel trace (the grid tells the two sequences apart)."""
    groups = {}
    for r in csv.DictReader(open(path)):
        if 'k_jf_' not in r.get('Kernel_Name', ''):
            continue
        name = 'k_jf_planes<%s>' % ('uint8' if 'unsigned char' in r['Kernel_Name'] else 'int32') if 'k_jf_planes' in r['Kernel_Name'] else 'k_jf_match'
        grid = 'x'.join(r.get('Grid_Size_' + a, '?') for a in 'XYZ')
        groups.setdefault((name, grid), []).append(int(r['End_Timestamp']) - int(r['Start_Timestamp']))
    with open(OUT, 'a') as f:
        f.write('# per kernel, from a separate `rocprofv3 --kernel-trace --stats -- python tools/jf_eval_time.py --score-only` run: 3 scoring calls of the\n'
                '# 480x854 / 20 frames / 2 objects sequence, then 3 of 1080x1920 / 8 frames / 8 objects (predictions = ground truth moved by (2, -3) px)\n')
        f.write('%-24s %-20s %6s %10s %10s %10s\n' % ('kernel', 'grid (work-items)', 'calls', 'median us', 'min us', 'max us'))
        for (name, grid), ns in groups.items():
            f.write('%-24s %-20s %6d %10.1f %10.1f %10.1f\n' % (name, grid, len(ns), statistics.median(ns) / 1e3, min(ns) / 1e3, max(ns) / 1e3))
    print('appended %d rows to %s' % (len(groups), OUT))


def main():
    torch.set_grad_enabled(False)
    prop = torch.cuda.get_device_properties(0)
    say('# J&F scoring on the GPU (csrc/jf_eval.hip) against the numpy path; box: %s (%s, %d CUs), %d host CPUs; %s' % (
        prop.name, getattr(prop, 'gcnArchName', '?').split(':')[0], prop.multi_processor_count, os.cpu_count(), time.strftime('%Y-%m-%d')))
    say('# host clock around whole j_and_f calls, median of %d alternating rounds after one warm-up call per arm; the values of both arms are equal' % ROUNDS)
    seq, big = sequences()
    labels, track_s = tracker_and_labels(seq)
    g, n = time_shape('480x854, 20 frames, 2 objects (tracker output)', labels, seq.gt, seq.obj_ids)
    say('Tracker.run_sequence on the same 480x854 sequence (ResNet-101, first-frame fit included), median of 3: %.1f ms; scoring it: GPU %.3f ms = %.3fx, '
        'numpy %.1f ms = %.1fx the tracking time' % (track_s * 1e3, g, g / (track_s * 1e3), n, n / (track_s * 1e3)))
    time_shape('480x854, 20 frames, 2 objects (gt moved 2,-3)', shifted(seq.gt), seq.gt, seq.obj_ids)
    time_shape('1080x1920, 8 frames, 8 objects (gt moved 2,-3)', shifted(big.gt), big.gt, big.obj_ids)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


if __name__ == '__main__':
    if '--score-only' in sys.argv:
        score_only()
    elif '--stats-csv' in sys.argv:
        append_stats(sys.argv[sys.argv.index('--stats-csv') + 1])
    else:
        main()
