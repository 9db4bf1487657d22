"""bench.py -- headline metric of BASELINE.json on synthetic data:

    segmented frames / sec / GPU  (480p, ResNet101, full CG iterations)

One "step" = one frame of a video sequence through the hot path (frame 0 = Tracker.initialize for every
object: augmentation, 5 trunk passes, joint GN/CG fit; frames >= 1 = Tracker.track: trunk, per-object
score + refinement, merge, memory insert, and every 8th frame a 10-iteration CG re-solve).  The timed region
is the reference's own definition of FPS (model/tracker.py:130,159-161): N frames / wall-clock of the
sequence loop, initialize() included, with a device sync on both sides.

    python bench.py --gpus 1 --steps 64 --warmup 8
    python bench.py --gpus 1 --steps 64 --warmup 8 --full     # + the add-on legs after the headline (N = 1 only)
    python bench.py --gpus 8 ...            # starts 8 ranks itself (torch.distributed.run, one process per GPU)

A plain run sets up, warms up, runs the timed repeats, writes --dump-outputs if asked and prints the line.  Everything else it can
measure runs only with --full, after the headline is complete: the initialize() sweep, the dataset leg, the streaming leg, the CG
roofline, the dominant kernel alone, the CPU oracle baseline and the dataset-level J&F against fixture G14 (the --no-<leg> options skip
single legs of it).

Workload = BASELINE.json configs[2] stand-in ("ResNet101 full-iteration optimizer, dv2017val multi-object"):
one "dv2017-like" synthetic sequence per rank, 480x854, 2 objects (the DAVIS-2017 val mean), memory 80, c=96.
No checkpoint / dataset exists on the box, so the weights are synthetic, built so that the tracker's feedback loop
closes like it does with trained weights (round-1 VERDICT weak #1):
  * trunk: seeded random weights with the last BatchNorm of every residual branch scaled by 0.25 (taps O(1-10) instead of 1e7);
  * refiner: seeded default init turned into a "score-following" stand-in for a trained refiner
    (lib/synthetic.py: make_score_following_refiner -- same architecture and arithmetic, confident masks where the target
    model's score exceeds 0.5), so that every tracked frame inserts a sample into the memory and every 8th frame re-solves
    the filter.  The line reports both counters and the run FAILS if they do not match the reference's schedule or if
    anything on the path is non-finite.
N > 1: one process per GPU (torch.distributed, RCCL only for the barrier + max-reduce of the wall time);
sequences are independent, so ranks never exchange data ("weak" scaling: one sequence per rank); every rank writes
``rank_<r>.json`` into --report-dir.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_TFLOPS = 157.3          # MI355X fp32 MFMA dense peak (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=64, help='frames in the timed sequence (frame 0 = initialize)')
    ap.add_argument('--warmup', type=int, default=8, help='untimed frames on a throw-away sequence')
    ap.add_argument('--repeats', type=int, default=5,
                    help='the timed region is run on this many FRESH sequences (other seeds, same length / objects) after the warm-up, each bracketed '
                         'by barrier + synchronize like one run; value = MEDIAN, min / max / all values are in the line (round-3 VERDICT: one 45 ms '
                         'sample is not a headline)')
    ap.add_argument('--backbone', default='resnet101')
    ap.add_argument('--objects', type=int, default=2)
    ap.add_argument('--size', default='480x854')
    ap.add_argument('--trunk-batch', type=int, default=16, help='frames per trunk pass (1 = frame by frame like the reference)')
    ap.add_argument('--trunk-lanes', type=int, default=2, help='concurrent sub-batches (streams) of a trunk pass')
    ap.add_argument('--fast', action='store_true', help='README "fast" schedule (fewer CG iterations)')
    ap.add_argument('--init-lanes', type=int, default=4, help='concurrent streams for the target-model fits of objects starting together')
    ap.add_argument('--no-windows', action='store_true', help='track frame by frame instead of one window per filter re-solve interval')
    ap.add_argument('--no-winograd', action='store_true', help='3x3 convs on the direct (halo) kernels only')
    ap.add_argument('--no-prefetch', action='store_true', help='dataset legs (--sequences, dataset_sim): preload each sequence before it is tracked instead of during the previous one')
    ap.add_argument('--no-winograd4', action='store_true', help='no Winograd F(4x4,3x3): the wide 3x3 convs stay on the fused F(2x2,3x3) kernel')
    ap.add_argument('--first-pass-overlap', action='store_true', help='first trunk pass on a side stream next to the fits of initialize()')
    ap.add_argument('--no-early-first-pass', action='store_true', help='first tracking trunk pass after initialize() instead of under its augmentation')
    ap.add_argument('--refiner-serial', action='store_true', help='refiner graph without parallel pyramid-level branches')
    ap.add_argument('--init-graph', action='store_true', help='first-frame fits replayed as one hipGraph per target model (default: launch by launch; no gain measured)')
    ap.add_argument('--no-persistent-cg', action='store_true', help='filter re-solves as 4 launches per CG iteration instead of one persistent launch')
    ap.add_argument('--random-refiner', action='store_true',
                    help='default-initialised refiner (round-1 workload: no mask ever exceeds 0.5, updates early-out; counters are reported, not asserted)')
    ap.add_argument('--full', action='store_true',
                    help='after the headline, run the add-on legs as well (N = 1 only): initialize() sweep, dataset leg, streaming leg, '
                         'CG roofline, dominant kernel, CPU baseline, dataset-level J&F.  The --no-<leg>, --cpu-frames, --init-sweep-counts, '
                         '--jf-draws and --no-oracle-spread options below act on these legs only')
    ap.add_argument('--no-oracle-spread', action='store_true', help='skip the second (untimed) oracle run that measures the oracle against itself')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-streaming', action='store_true', help='skip the streaming leg (Tracker.track frame by frame: what an online caller gets)')
    ap.add_argument('--no-jf-fixture', action='store_true', help='skip the dataset-level J&F leg (fixture G14 tracked on the HIP path, ~40 s)')
    ap.add_argument('--init-sweep-counts', default='1,2,5', help='object counts of the initialize() sweep')
    ap.add_argument('--jf-draws', type=int, default=4, help='dataset runs of the HIP path in the J&F leg (stem weights moved by 0 .. n-1 ulp; the gate in tests/ uses 8)')
    ap.add_argument('--no-cg-roofline', action='store_true', help='skip the CG roofline leg (profiling runs: the trace then ends with the timed region)')
    ap.add_argument('--no-init-sweep', action='store_true', help='skip the initialize() timing for 1/2/5 objects')
    ap.add_argument('--cpu-frames', type=int, default=12, help='tracked frames of the CPU baseline sample (bounded to ~30 s)')
    ap.add_argument('--no-window-inserts', action='store_true', help='memory inserts frame by frame (3 launches per frame and object) instead of one batched update per window')
    ap.add_argument('--pull-push-fill', action='store_true', help="first-frame hole fill by the device-side pull-push pyramid (ImageAugmenter(fill='pull_push'), rounds 2-5) instead of Telea's method on the host (the reference's recipe restated; default since round 6)")
    ap.add_argument('--refiner-graph', action='store_true', help='refiner windows replayed as hipGraphs (Tracker(refiner_graphs=True); opt-in since round 6: the default launches them kernel by kernel with the deep levels on a side stream -- same speed, profiles/r06_refiner_window_ab.txt)')
    ap.add_argument('--no-refiner-graph', action='store_true', help='(the default since round 6; kept so that older command lines still parse)')
    ap.add_argument('--trunk-graph', action='store_true', help='trunk passes replayed as hipGraphs instead of launched kernel by kernel (no gain measured)')
    ap.add_argument('--no-fold-tail', action='store_true', help='a last trunk batch of 1-3 frames stays a pass of its own instead of joining the one before it')
    ap.add_argument('--balance', action='store_true', help='trunk batches of similar size instead of full ones and a short tail pass (measured slower at 20 frames)')
    ap.add_argument('--pipeline', action='store_true', help='two tap sets, trunk passes one ahead on a side stream, one beside the first-frame fits (measured: +4 %% frames/s at 20 frames, trunk passes 5 %% slower)')
    ap.add_argument('--first-batch', type=int, default=0, help='frames of the pipelined first trunk pass (default: trunk batch / 2)')
    ap.add_argument('--overlap', action='store_true', help='run the next trunk batch on a side stream, overlapped with tracking')
    ap.add_argument('--memory', type=int, default=80, help='target-model memory slots (80 = evaluate.py:80)')
    ap.add_argument('--late-object', type=int, default=None, help='frame at which the last object first appears')
    ap.add_argument('--dist-backend', default='nccl', help='nccl (= RCCL) for real multi-GPU runs; gloo to exercise the path on one GPU')
    ap.add_argument('--share-gpu', action='store_true', help='testing only: all ranks use cuda:0')
    ap.add_argument('--launch-check', action='store_true',
                    help='exercise only the multi-process machinery (self-launch, process group, barrier, max-reduce, rank reports) with a '
                         'stub workload; needs no GPU with --dist-backend gloo (CPU test of the N > 1 path)')
    ap.add_argument('--sequences', type=int, default=0,
                    help='sharded (strong-scaling) mode, BASELINE config 4 shape: S dv2017-like synthetic sequences (1-5 objects, 34-104 frames) are '
                         'sharded over the ranks, length-balanced; value = sum of frames / max rank wall time')
    ap.add_argument('--shard-warm', action='store_true', help='sharded mode: run the rank\'s share once untimed first, so that the timed pass is the steady state (every shape seen, allocator warm)')
    ap.add_argument('--no-dataset-sim', action='store_true', help='skip the dataset-level leg (30 dv2017-like sequences through the same tracker, N = 1 only)')
    ap.add_argument('--no-cpu-pin', action='store_true', help='leave the host threads to the scheduler instead of pinning them to cores near the GPU')
    ap.add_argument('--no-pin', action='store_true', help='do not restrict every rank to its own GPU through HIP_VISIBLE_DEVICES')
    ap.add_argument('--debug-allocs', action='store_true', help='print the Python stacks of device allocations (hipMalloc) made inside the timed region')
    ap.add_argument('--report-dir', default=None,
                    help='where every rank writes rank_<r>.json (default: a new directory in the system temp dir for every launch, shared by its '
                         'ranks; the checkout itself may be read-only)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed repeats, write what the last one returned for its last frame (the label image a caller of '
                         'Tracker.run_sequence receives) as DIR/<name>.npy in float32: same arguments, same inputs, so two builds compare '
                         'output for output (rank 0, single-sequence mode only)')
    args = ap.parse_args(argv)
    if args.dump_outputs and args.sequences > 0:
        ap.error('--dump-outputs needs the single-sequence mode (no --sequences)')
    return args


def default_report_dir():
    """A fresh directory for the rank reports of one launch.  Ranks started by bench.py itself get theirs from self_launch; ranks started by
    an outside launcher have no common parent and agree on a name keyed by user and rendezvous (every rank rewrites its own rank_<r>.json
    before any rank reads it, and only ranks 0 .. world-1 are read, so files of an earlier launch under the same name are never used)."""
    import tempfile
    if 'WORLD_SIZE' not in os.environ:
        return tempfile.mkdtemp(prefix='frtm_bench_ranks_')
    launch = '%s_%s' % (os.environ.get('TORCHELASTIC_RUN_ID', 'run'), os.environ.get('MASTER_PORT', 'port'))
    return os.path.join(tempfile.gettempdir(), 'frtm_bench_ranks_%d_%s' % (os.getuid(), launch))


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """arrays: name -> tensor.  Each is written as out_dir/<name>.npy in float32; all of them together stay under DUMP_MAX_BYTES (a larger
    array is replaced by a fixed, seeded sample of its elements, written with the flat indices of the sample as <name>_index.npy)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    budget = DUMP_MAX_BYTES // max(len(arrays), 1) // 2
    files = []
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy().astype(np.float32).reshape(t.shape)
        if a.nbytes > budget:
            idx = np.sort(np.random.default_rng(0).choice(a.size, size=budget // 8, replace=False))
            np.save(os.path.join(out_dir, name + '_index.npy'), idx.astype(np.float64))
            files.append(name + '_index.npy')
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, name + '.npy'), a)
        files.append(name + '.npy')
    return files


# ------------------------------------------------------------------------------------------------------------------
# multi-GPU launch: `python bench.py --gpus N` starts N ranks itself (one process per GPU)
# ------------------------------------------------------------------------------------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


def self_launch(args):
    """Re-executes this script under torch.distributed.run with --nproc-per-node = --gpus.  Rank 0 prints the JSON line;
    the children's stdout / stderr pass straight through."""
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', '8')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(args.gpus),
           '--master-addr', '127.0.0.1', '--master-port', str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    if args.report_dir is None:                 # one new directory for the ranks of this launch
        cmd += ['--report-dir', default_report_dir()]
    return subprocess.call(cmd, env=env)



def init_dist(backend, world, dev=None, nccl_timeout_s=180):
    from frtm_vos_amd.shard import init_process_groups
    return init_process_groups(backend, world, dev, nccl_timeout_s)


class StageTimer:
    """HIP events on torch's current stream (the stream every frtm_* kernel is enqueued on)."""

    def __init__(self):
        self.spans = {}

    def wrap(self, name, fn):
        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.spans.setdefault(name, []).append((e0, e1))
            return out
        return timed

    def totals(self):
        return {k: (sum(a.elapsed_time(b) for a, b in v), len(v)) for k, v in self.spans.items()}

    def reset(self):
        self.spans = {}


def run_sequence(tracker, seq):
    """The reference's per-sequence loop (model/tracker.py:103-163), label decoding included, PNG writing not (that is
    run_dataset's part, outside the reference's timed region as well).  Returns the label images."""
    outputs, _ = tracker.run_sequence(seq)
    return outputs


def synthetic_refiner(args, chans):
    """The refiner both legs use: seeded default init (seed 1) + the score-following edit."""
    from frtm_vos_amd.lib.synthetic import make_score_following_refiner
    from frtm_vos_amd.model.seg_network import SegNetwork
    torch.manual_seed(1)
    net = SegNetwork(1, 64, chans, True).eval()
    return net if args.random_refiner else make_score_following_refiner(net)


# ------------------------------------------------------------------------------------------------------------------
# checks on the timed run: counters of the per-frame update work, finiteness, tracking quality
# ------------------------------------------------------------------------------------------------------------------

def path_counters(tracker, seq, n_frames):
    """Memory inserts and filter re-solves the timed sequence performed (device-side counters of the slot kernel + host
    counters of Discriminator.update) next to what the reference's schedule asks for (discriminator.py:208-227: one insert per
    tracked frame, one re-solve on every frame with frame_num % train_skipping == 0), and finiteness of everything the
    target models hold."""
    inserts = skipped = solves = early = sched_ins = sched_solve = 0
    finite = True
    aborts = 0
    for obj_id, t in tracker.targets.items():
        d = t.discriminator
        aborts += d.num_persistent_aborts + int(d.recover_from_abort())
        tracked = n_frames - 1 - seq.start_frame(obj_id)
        sched_ins += tracked
        sched_solve += tracked // d.train_skipping
        a, b = d.memory.insert_counts
        inserts, skipped = inserts + a, skipped + b
        solves += d.num_solves
        early += d.num_early_outs
        for x in (d.project.weight, d.filter.weight, d.memory.samples, d.memory.normal_B, d.memory.normal_c, d.memory.weights):
            finite = finite and bool(torch.isfinite(x).all())
    finite = finite and bool(torch.isfinite(tracker.current_masks).all())
    return {'memory_inserts': inserts, 'memory_inserts_scheduled': sched_ins, 'cg_solves': solves, 'cg_solves_scheduled': sched_solve,
            'early_outs_fewer_than_10_px': skipped + early, 'cg_persistent_aborts': aborts, 'all_finite': finite}


def tracking_quality(outputs, seq):
    """Mean IoU of the decoded label images against the synthetic ground truth (frames after each object's start frame)."""
    ious = []
    for obj in seq.obj_ids:
        for t in range(seq.start_frame(obj) + 1, len(outputs)):
            a, b = outputs[t].reshape(-1) == obj, seq.gt[t].reshape(-1).to(outputs[t].device) == obj
            u = int((a | b).sum())
            if u:
                ious.append(float((a & b).sum()) / u)
    return sum(ious) / max(len(ious), 1)


# ------------------------------------------------------------------------------------------------------------------
# CPU baseline: the oracle on the host cores, SAME sequence / objects / schedule / refiner weights
# ------------------------------------------------------------------------------------------------------------------

def cpu_baseline(args, size, seq_cpu, aug_stacks, n_frames, gpu_labels=None):
    """oracle/cpu_ref.py ('port') on the host cores: the first 1 + n_frames frames of the SAME synthetic sequence the GPU leg
    timed (same objects, iteration schedule, trunk and refiner weights).  Augmentation: the oracle has no augmenter (OpenCV /
    NPP are absent); the augmented first-frame stacks the GPU leg produced are replayed, their generation is NOT in the CPU time."""
    from oracle import cpu_ref as O
    P = O.resnet_random_params(args.backbone, seed=0)
    cin = {'resnet101': 1024, 'resnet50': 1024, 'resnet18': 256, 'resnet34': 256}[args.backbone]
    chans = {'layer5': cin * 2, 'layer4': cin, 'layer3': cin // 2, 'layer2': cin // 4}
    refiner = synthetic_refiner(args, chans)
    iters = ((5, 10, 10, 10), (5,)) if args.fast else ((5, 10, 10, 10, 10), (10,))
    ncpu = os.cpu_count()
    # thread count that serves the oracle best on this host: 16 or 32 (more only loses: 64 threads are slower, all 256 of the GPU
    # box's cores took minutes for ONE ResNet-101 frame); probed on a quarter-size frame, untimed
    probe = seq_cpu[0][0].unsqueeze(0)[..., ::2, ::2].contiguous()
    best = None
    with torch.no_grad():
        for th in sorted({min(16, ncpu), min(32, ncpu)}):
            torch.set_num_threads(th)
            O.resnet_forward(args.backbone, P, probe, ['layer4'])
            t0 = time.time()
            O.resnet_forward(args.backbone, P, probe, ['layer4'])
            dt = time.time() - t0
            if best is None or dt < best[0]:
                best = (dt, th)
    threads = best[1]
    torch.set_num_threads(threads)
    _phase('oracle thread probe done (%d threads)' % threads)
    n_obj = len(seq_cpu.obj_ids)
    start_w = []
    for k in range(n_obj):                                  # the draws of the GPU leg, repeated (same seeds, same order: project, filter)
        torch.manual_seed(4242 if k == 0 else 0)
        pj = torch.nn.Conv2d(cin, 96, 1, bias=False)       # on the host, from the global CPU generator: the reference's draw (discriminator.py:86-87)
        fl = torch.nn.Conv2d(96, 1, 3, padding=1, bias=False)
        start_w.append((pj.weight.detach().clone(), fl.weight.detach().clone()))
    def leg(budget_s):
        """initialize() + tracked frames of the oracle; returns (labels, frames done, memory inserts, seconds)."""
        t0 = time.time()
        with torch.no_grad():
            discs = []
            for k in range(n_obj):
                w1, w2 = start_w[k]
                d = O.DiscriminatorRef(w1, w2, init_iters=iters[0], update_iters=iters[1], CG_forgetting_rate=750, memory_size=args.memory,
                                       pixel_weighting=dict(method='hinge', tf=0.1))
                im, msk = aug_stacks[k]
                d.init(O.resnet_forward(args.backbone, P, im, ['layer4'])['layer4'], msk)
                discs.append(d)
            done, inserts = 1, 0
            labels = [seq_cpu.gt[0].reshape(size).clone()]
            for t in range(1, n_frames + 1):
                if time.time() - t0 > budget_s:   # bounded sample
                    break
                done += 1
                im = seq_cpu[t][0]
                taps = O.resnet_forward(args.backbone, P, im)
                scores = torch.cat([d.apply(taps['layer4']) for d in discs])
                y = torch.sigmoid(refiner(scores, taps, im.shape[-2:]))
                masks = torch.zeros(n_obj + 1, *im.shape[-2:])
                masks[1:] = y[:, 0]
                masks = O.merge_masks(masks)
                labels.append(O.merge_masks(masks).argmax(0).to(torch.uint8))        # label decoding of tracker.py:146-150
                for k, d in enumerate(discs):
                    if int((masks[k + 1] > 0.5).sum()) >= 10:
                        inserts += 1
                    d.update(masks[k + 1][None, None])
        return labels, done, inserts, time.time() - t0

    cpu_labels, done, inserts, T = leg(30.0)              # ~30 s of CPU work at most
    _phase('oracle leg done')
    parity = None
    if gpu_labels is not None and done > 3:
        # J&F (DAVIS measures, lib/davis.py pinned to the reference by fixture G10) of BOTH paths against the synthetic ground truth
        # on the frames the CPU leg covered: the north star asks for the two within +-0.1 points
        from frtm_vos_amd.lib.evaluation import j_and_f
        ids = list(seq_cpu.obj_ids)
        gt = [seq_cpu.gt[t].reshape(size).numpy() for t in range(done)]
        jf_g = j_and_f([gpu_labels[t].reshape(size).cpu().numpy() for t in range(done)], gt, ids)
        jf_c = j_and_f([cpu_labels[t].numpy() for t in range(done)], gt, ids)
        agree = float(sum(float((gpu_labels[t].reshape(size).cpu() == cpu_labels[t]).float().mean()) for t in range(1, done)) / (done - 1))
        parity = {'frames': done, 'J&F_hip_path': round(jf_g[0], 3), 'J&F_cpu_oracle': round(jf_c[0], 3), 'abs_diff_points': round(abs(jf_g[0] - jf_c[0]), 3),
                  'label_agreement': round(agree, 5)}
        # How far is the oracle from ITSELF?  The same leg once more with half the threads (another summation order in its convs
        # and reductions: the truncated GN/CG fits amplify that, oracle/make_golden_r2.py: spread).  Not timed, same frames.
        if T < 25.0 and threads > 1 and not args.no_oracle_spread:
            torch.set_num_threads(max(1, threads // 2))
            other, done2, _, _ = leg(60.0)
            torch.set_num_threads(threads)
            m = min(done, done2)
            jf_o = j_and_f([other[t].numpy() for t in range(m)], gt[:m], ids)
            jf_c_m = j_and_f([cpu_labels[t].numpy() for t in range(m)], gt[:m], ids)
            parity['oracle_vs_itself_half_threads'] = {
                'J&F': round(jf_o[0], 3), 'abs_diff_points': round(abs(jf_o[0] - jf_c_m[0]), 3),
                'label_agreement': round(float(sum(float((other[t] == cpu_labels[t]).float().mean()) for t in range(1, m)) / max(m - 1, 1)), 5)}
    return {'value': done / T, 'unit': 'frames/s', 'cores': threads, 'kind': 'port', 'jf_parity_vs_hip_path': parity,
            'sample': 'oracle/cpu_ref.py on the same synthetic sequence as the GPU leg: %s %dx%d, %d objects, %s iterations, same trunk / '
                      'refiner weights, initialize() (augmented stacks replayed from the GPU leg, their generation not timed) + %d tracked '
                      'frames (%d memory inserts), %d torch threads (faster of 16 / 32 on a trunk probe) of %d host cores, %.1f s' %
                      (args.backbone, size[0], size[1], n_obj, 'fast' if args.fast else 'full', done - 1, inserts, threads, ncpu, T)}


def streaming_leg(tracker, seq, dev, n_frames=40):
    """What an ONLINE caller gets (round-3 VERDICT "Next" #9): frames arrive one at a time and go through Tracker.track(image) -- trunk on
    ONE frame, scores, refiner, merge, memory insert, every 8th frame the re-solve -- with the tracker's default kernels and the streaming
    options (``Tracker.streaming``: single-frame trunk pass and per-frame refiner replayed from hipGraphs).  Two numbers: throughput (frames
    enqueued back to back, one synchronise at the end) and latency (a synchronise after every frame: time from the frame's arrival to its
    masks).  initialize() is outside (it is the same as in the headline)."""
    frames = [seq[t][0] for t in range(len(seq.images))][:n_frames + 1]
    tracker.release_targets()
    tracker.clear()
    own = torch.cuda.Stream(device=dev)
    out = {}
    with torch.cuda.stream(own):
        im, lb, ids = seq[0]
        tracker.current_frame = 0
        tracker.initialize(im, lb, ids)
        tracker.current_frame = 1
        for mode in ('warm', 'throughput', 'latency'):
            torch.cuda.synchronize()
            t0 = time.time()
            lat = []
            for im in frames[1:]:
                t1 = time.time()
                tracker.track(im)
                tracker.current_frame += 1
                if mode == 'latency':
                    own.synchronize()
                    lat.append(time.time() - t1)
            own.synchronize()
            T = time.time() - t0
            if mode == 'throughput':
                out['streaming_fps'] = round((len(frames) - 1) / T, 1)
            elif mode == 'latency':
                lat.sort()
                out['latency_ms_median'] = round(1e3 * lat[len(lat) // 2], 3)
                out['latency_ms_p90'] = round(1e3 * lat[int(0.9 * (len(lat) - 1))], 3)
    torch.cuda.current_stream().wait_stream(own)
    tracker.release_targets()
    tracker.clear()
    out['frames'] = len(frames) - 1
    out['note'] = 'Tracker.track(image) frame by frame (no pre-loaded sequence, no trunk batch, no tracking windows); 2 objects, full update schedule'
    return out


def jf_vs_fixture(dev, draws=4):
    """Dataset-level J&F parity in the driver's line (round-3 VERDICT "Next" #1): fixture G14's synthetic dataset (BASELINE config 3's shape:
    32 sequences x 40 frames, 1-5 objects, 77 objects, ResNet-101, full schedule, memory 80) is tracked on the HIP product path with the
    fixture's start weights / augmentation / refiner and evaluated with the G10-pinned DAVIS measures; the CPU side is NOT re-run here: the
    fixture holds the float32 oracle's per-object J / F (oracle/make_golden_jf.py --spec v2) at four thread counts and with its stem
    weights moved by 1 / 3 ulp (the single-run noise of the REFERENCE arithmetic) and its float64 run.  The HIP side is tracked `draws`
    times, stem weights moved by K = 0 .. draws-1 ulp (K = 0: the build as it ships): the +-0.1 bar is a statement about expectations --
    one dataset-level run of EITHER implementation moves by ~0.05 (1 sigma) under such perturbations (tests/test_north_star_gpu.py runs
    eight draws and gates on it).  Part of the cpu_baseline leg (the only place bench.py may touch oracle/)."""
    import copy
    from concurrent.futures import ProcessPoolExecutor
    import numpy as np
    import oracle.make_golden_jf as JF
    from oracle.tracker_ref import shift_flip_augment
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    G = os.path.join(ROOT, 'tests', 'golden')
    fx = np.load(os.path.join(G, 'g14_jf_float32.npz'))
    specs = [tuple(int(v) for v in row) for row in fx['specs']]
    params = Parameters(None, fast=False, device=dev, feature_extractor='resnet101')
    refiner = JF.refiner_for('resnet101')
    params.refiner_factory = lambda chans: copy.deepcopy(refiner)
    params.disc_params.update(**JF.DISC)
    trk = params.get_model().eval()
    trk.augment = shift_flip_augment
    ext = trk.feature_extractor
    stem = ext.resnet.conv1.weight.data.clone()
    # Tracking first, evaluation afterwards, in workers of a FORK SERVER: forking this process while it drives the GPU (a ProcessPoolExecutor
    # forks on demand, inside submit()) cost 170 ms per worker and slowed the tracking loop 15x (copy-on-write faults and the driver's
    # notifiers on a 30 GB address space: 50 s instead of 3 s per dataset run, tools/jf_leg_timing.py).
    import multiprocessing as mp
    jobs = []
    seqs = []                    # rendered once, resident on the GPU for all draws (1.6 GB)
    for k, (n_frames, n_obj, seed) in enumerate(specs):
        seqs.append(SyntheticSequence('jg%02d' % k, n_frames, JF.SIZE, n_obj, seed=seed))
        seqs[-1].preload(dev)
    t0 = time.time()
    for di in range(max(1, int(draws))):
        ext.resnet.conv1.weight.data.copy_(stem * (1.0 + di * 2.0 ** -23))
        ext.upload()
        for k, (n_frames, n_obj, seed) in enumerate(specs):
            trk.start_weights = lambda oid, s=seed: JF.start_weights(s, oid)
            labels, _ = trk.run_sequence(seqs[k])
            jobs.append(((di, k), 'jg%02d' % k, torch.stack([l.reshape(JF.SIZE) for l in labels]).cpu().numpy(), n_frames, n_obj, seed))
    torch.cuda.synchronize()
    t_track = time.time() - t0
    for seq in seqs:
        seq.release()
    ext.resnet.conv1.weight.data.copy_(stem)
    ext.upload()
    with ProcessPoolExecutor(max_workers=min(32, max(1, (os.cpu_count() or 8) // 2)), mp_context=mp.get_context('forkserver')) as ex:
        res = {key: np.array(v) for key, v in ex.map(JF.jf_job, jobs)}
    hips = [np.concatenate([res[(di, k)] for k in range(len(specs))]).mean(1) * 100 for di in range(max(1, int(draws)))]
    hip = hips[0]
    ora = np.concatenate([fx['jf_%d' % k] for k in range(len(specs))]).mean(1) * 100
    others = {}
    for name in ('float32_t2', 'float32_t3', 'float32_t6', 'float32_p1', 'float32_p3', 'float64'):
        f = os.path.join(G, 'g14_jf_%s.npz' % name)
        if os.path.exists(f):
            o = np.load(f)
            if all(('jf_%d' % k) in o for k in range(len(specs))):
                others[name] = np.concatenate([o['jf_%d' % k] for k in range(len(specs))]).mean(1) * 100
    o_draws = [ora] + [v for n_, v in others.items() if n_.startswith('float32')]
    o_vals = np.array([float(v.mean()) for v in o_draws])
    h_vals = np.array([float(v.mean()) for v in hips])
    o_mean_obj = np.mean(o_draws, axis=0)
    # The oracle's single-run sigma: sequences are tracked independently, so the variance of a dataset-level run is the sum of the per-sequence
    # variances, each from ALL the oracle draws of that sequence (the full runs above + fixture G16: sixteen more draws of the two sequences that
    # carry the spread -- oracle/make_golden_jf_draws.py).  The default build's distance to the oracle's mean is quoted in these sigmas.
    nobj = [n_obj for _, n_obj, _ in specs]
    starts = np.cumsum([0] + nobj)
    var_o, extra = 0.0, {}
    for k in range(len(specs)):
        rows = [v[starts[k]:starts[k + 1]].sum() for v in o_draws]
        f = os.path.join(G, 'g16_jf_draws_seq%d.npz' % k)
        if os.path.exists(f):
            e_ = np.load(f)['jf']
            rows += [100 * float(r.mean(1).sum()) for r in e_]
            extra['jg%02d' % k] = len(rows)
        var_o += float(np.var(rows, ddof=1))
    sig_o = float(np.sqrt(var_o)) / float(sum(nobj))
    out = {'fixture': 'tests/golden/g14_jf_float32*.npz (32 sequences x 40 frames, %d objects; float32 CPU oracle: %d recorded runs)' % (len(ora), len(o_draws)),
           'J&F_hip_path_mean_of_draws': round(float(h_vals.mean()), 3), 'J&F_cpu_oracle_f32_mean_of_runs': round(float(o_vals.mean()), 3),
           'diff_points': round(float(h_vals.mean() - o_vals.mean()), 3),
           'hip_draws_stem_weights_moved_by_K_ulp': [round(float(v), 3) for v in h_vals],
           'oracle_f32_runs': {'float32_t4': round(float(ora.mean()), 3), **{n_: round(float(v.mean()), 3) for n_, v in others.items() if n_.startswith('float32')}},
           'oracle_f64': round(float(others['float64'].mean()), 3) if 'float64' in others else None,
           'single_run_noise_floor_points': {'oracle_f32_range': round(float(o_vals.max() - o_vals.min()), 3), 'hip_range': round(float(h_vals.max() - h_vals.min()), 3)},
           'oracle_single_run_sigma_points': {'value': round(sig_o, 3), 'method': 'sqrt(sum of per-sequence variances) over all recorded oracle draws', 'draws_of_sequences_with_extra_runs': extra},
           'default_build_vs_oracle_mean': {'diff_points': round(float(hip.mean() - o_vals.mean()), 3), 'in_oracle_sigmas': round(float((hip.mean() - o_vals.mean()) / sig_o), 2),
                                            'oracle_run_range': [round(float(o_vals.min()), 3), round(float(o_vals.max()), 3)]},
           'default_build_vs_oracle_4_threads': {'diff_points': round(float(hip.mean() - ora.mean()), 3),
                                                 'per_object_abs_diff_mean': round(float(np.abs(hip - ora).mean()), 3),
                                                 'per_object_abs_diff_max': round(float(np.abs(hip - ora).max()), 2),
                                                 'per_object_median_diff': round(float(np.median(hip - ora)), 3)},
           'per_object_median_diff_to_oracle_mean_per_draw': [round(float(np.median(h - o_mean_obj)), 3) for h in hips],
           'hip_tracking_seconds': round(t_track, 1),
           'note': 'HIP side tracked here (draws x 1280 frames); the oracle side is the recorded fixture.  North star: +-0.1 points, tested on the '
                   'means (one dataset-level run of either implementation is a random variable under ulp-level perturbations: object 1 of the five-object '
                   'sequence jg04 is fully occluded on frames 7-15 and how much of it is recovered on frame 16 is decided at rounding level -- 39-50 points '
                   'over 22 runs of the float32 oracle, 41-49 over 16 of the HIP path, profiles/r05_jf_branch.txt).'}
    return out


def cg_roofline(dev, size, n_samples=80, c=96, iters=10, reps=20, persistent=True):
    """HBM-bound leg: GaussNewtonCG.run((10,)) of the filter-only problem on a full memory (N = 80, 30x54 grid, c = 96).
    Algorithmic bytes: reference formulation 2*4*N*c*hw + 4*N*HW per operator application (+4*N*HW labels for
    the right-hand side); this formulation's own traffic 2*4*N*c*hw + 4*N*10*hw.  11 applications per run."""
    from frtm_vos_amd.lib.tensorlist import TensorList
    from frtm_vos_amd.model.discriminator import DiscriminatorLoss
    from frtm_vos_amd.model.memory import Memory
    from frtm_vos_amd.model.optimizer import GaussNewtonCG
    Hh, Ww = size
    h, w = (Hh + 15) // 16, (Ww + 15) // 16
    g = torch.Generator().manual_seed(7)
    mem = Memory(n_samples, (c, h, w), (1, Hh, Ww), dev, 0.1, pixel_weighting=dict(method='hinge', tf=0.1))
    mem.samples.copy_(torch.relu(torch.randn(n_samples, c, h, w, generator=g)))
    lab = torch.zeros(8, 1, Hh, Ww)
    lab[:, :, Hh // 4: Hh // 2, Ww // 4: Ww // 2] = 0.9
    for k in range(0, n_samples, 8):
        mem._build_normals(lab.to(dev), None, 8, None, k)
    mem.weights.fill_(1.0 / n_samples)
    mem.current_size = n_samples
    wv = torch.nn.Parameter(((torch.rand(1, c, 3, 3, generator=g) * 2 - 1) / 29.4).to(dev), requires_grad=False)
    opt = GaussNewtonCG(DiscriminatorLoss(mem, (1e-2,), (1e-2,), wv), TensorList([wv]), fletcher_reeves=False,
                        direction_forget_factor=0.9 ** 750)
    opt.persistent = persistent
    for _ in range(3):
        opt.run((iters,))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        opt.run((iters,))
    e1.record()
    torch.cuda.synchronize()
    ms_eager = e0.elapsed_time(e1) / reps
    g_ = torch.cuda.CUDAGraph()                      # the same run as one hipGraph: device time without host launch cost
    with torch.cuda.graph(g_):
        opt.run((iters,))
    g_.replay()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        g_.replay()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    hw, HW, apps = h * w, Hh * Ww, iters + 1
    ref_bytes = apps * (2 * 4 * n_samples * c * hw + 4 * n_samples * HW) + 4 * n_samples * HW
    own_bytes = apps * (2 * 4 * n_samples * c * hw + 4 * n_samples * 10 * hw)
    assert not opt.poll_persistent_abort(), 'persistent CG launch timed out'
    path = ('k_cg_run_persistent (one launch: features resident in registers)' if (persistent and opt._persistent_plan() is not None)
            else 'k_filter_scores + k_stencil + k_filter_wgrad + k_cg_step_small (4 launches per CG iteration)')
    resident = persistent and opt._persistent_plan() is not None
    # HBM-side bytes the run REALLY moves, from the committed PMC passes (profiles/r02_cg_traffic.json: the persistent launch reads the
    # features once, 155 MB per run; the multi-kernel chain re-reads them twice per operator application, 1.21 GB per run)
    measured = None
    tf = os.path.join(ROOT, 'profiles', 'r02_cg_traffic.json')
    if os.path.exists(tf):
        try:
            ks = json.load(open(tf))['kernels']
            if resident:
                k = [v for n_, v in ks.items() if 'k_cg_run_persistent' in n_][0]
                measured = k['fetch_bytes_per_launch'] + k['write_bytes_per_launch']
            else:
                measured = sum((v['fetch_bytes_per_launch'] + v['write_bytes_per_launch']) * v['launches'] for n_, v in ks.items()
                               if 'k_cg_run_persistent' not in n_) / max(1, [v for n_, v in ks.items() if 'k_vec_reduce_slabs' in n_][0]['launches'])
        except Exception:
            measured = None
    # FLOPs the run executes: per operator application the 3x3 score pass and the 3x3 weight gradient over the memory (2 * N * c * 9 * hw
    # each, scalar fp32 FMAs on the VALU) + the 9-point stencil (2 * N * 10 * hw); `apps` applications per run
    flops = apps * (2 * 2 * n_samples * c * 9 * hw + 2 * n_samples * 10 * hw)
    tf = flops / (ms * 1e-3) / 1e12
    hbm_eq = {'note': "SURVEY 8d's byte model (features streamed twice per operator application); the resident launch does NOT move these bytes -- "
                      "kept for continuity with rounds 1-3, not a roofline fraction of this kernel",
              'bytes_this_formulation': own_bytes, 'equivalent_rate_GBs': own_bytes / (ms * 1e-3) / 1e9,
              'bytes_reference_formulation': ref_bytes, 'equivalent_rate_on_reference_bytes_GBs': ref_bytes / (ms * 1e-3) / 1e9,
              'frac_on_reference_bytes': ref_bytes / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS}
    if resident:
        # round-3 VERDICT weak #6: the features stay in registers, so the step is VALU + grid-barrier bound -- quote it against the fp32
        # VECTOR peak (157.3 TFLOP/s, MI355X_MICROARCH.md) and give the HBM rate the launch really sustains next to it
        return {'bound': 'valu', 'kernel': 'GaussNewtonCG.run((10,)) of the filter problem, N=80: ' + path,
                'achieved': tf, 'peak': PEAK_F32_TFLOPS, 'unit': 'TFLOP/s', 'frac': tf / PEAK_F32_TFLOPS, 'flops_per_run': flops,
                'note': 'fp32 VALU FMAs (scores + weight gradient from register-resident features) + 2 XCD-hierarchical grid barriers per operator '
                        'application (22 per run); HBM traffic is the features ONCE per run',
                'measured_hbm_bytes_per_run': measured, 'measured_hbm_rate_GBs': None if measured is None else measured / (ms * 1e-3) / 1e9,
                'measured_hbm_frac_of_peak': None if measured is None else measured / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
                'ms_per_run': ms, 'ms_per_run_eager_launch': ms_eager, 'hbm_equivalents': hbm_eq}
    return {'bound': 'hbm', 'kernel': 'GaussNewtonCG.run((10,)) of the filter problem, N=80: ' + path,
            'achieved': own_bytes / (ms * 1e-3) / 1e9, 'peak': PEAK_HBM_GBS, 'unit': 'GB/s', 'frac': own_bytes / (ms * 1e-3) / 1e9 / PEAK_HBM_GBS,
            'measured_hbm_bytes_per_run': measured, 'measured_hbm_rate_GBs': None if measured is None else measured / (ms * 1e-3) / 1e9,
            'ms_per_run': ms, 'ms_per_run_eager_launch': ms_eager, 'valu_tflops': tf, 'hbm_equivalents': hbm_eq}


def dominant_kernel_leg(dev, frames=8, hw=(30, 54), reps=40):
    """roofline.dominant_kernel (VERDICT r5 'Next' #4): the trunk's dominant kernel -- k_conv_igemm<64,64,2,4,1> and its persistent form, the 1x1 GEMMs of ResNet-101's layer3
    (reference model/feature_extractor.py:50-65) -- ALONE on the GPU, measured in this run: its two shapes at one lane's batch (8 frames, 30x54) as
    `reps` back-to-back launches between HIP events on the stream they are launched on (BN + residual + ReLU resp. BN + ReLU fused, as in the trunk),
    with the shader clock read by a one-wave probe on a side stream under the same load (frtm_clock_probe: s_memtime against the 100 MHz counter)."""
    import ctypes
    from frtm_vos_amd import _hip as H, ops
    g = torch.Generator(device='cpu').manual_seed(11)
    out = {'name': 'k_conv_igemm_p (256->1024: the persistent form of k_conv_igemm<64,64,2,4,1>, round 6) / k_conv_igemm<64, 64, 2, 4, 1, 32> (1024->256: 812 tiles, below 1.5 per resident workgroup)', 'batch': frames, 'map': '%dx%d' % hw, 'launches_timed': reps, 'shapes': {}}
    side = torch.cuda.Stream(device=dev)
    clk = torch.zeros(2, dtype=torch.int64, device=dev)
    tot_fl, tot_us = 0.0, 0.0
    for cin, cout, with_res in ((256, 1024, True), (1024, 256, False)):
        x = torch.randn(frames, cin, hw[0], hw[1], generator=g).to(dev)
        wT, ktab, lay = ops.pack_weights((torch.randn(cout, cin, 1, 1, generator=g) * (1.0 / cin ** 0.5)).to(dev))
        sc, sh = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
        res = torch.randn(frames, cout, hw[0], hw[1], generator=g).to(dev) if with_res else None
        y = torch.empty(frames, cout, hw[0], hw[1], device=dev)

        def run(n):
            for _ in range(n):
                ops.conv2d(x, wT, cout, 1, 1, 0, ktab=ktab, scale=sc, shift=sh, relu=True, out=y, w_layout=lay, residual=res, tile=4)    # FRTM_TILE_64x64_8W: the planner's choice here
        run(8)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(reps)
        e1.record()
        torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / reps
        # the clock under this load: probe for ~0.6 x the sequence's length on a side stream, started behind the first launches
        probe_us = max(200, int(0.6 * us * reps))
        side.wait_stream(torch.cuda.current_stream())
        run(4)
        with torch.cuda.stream(side):
            H.lib().frtm_clock_probe(probe_us, ctypes.c_void_p(clk.data_ptr()), ctypes.c_void_p(side.cuda_stream))
        run(reps)
        torch.cuda.synchronize()
        cyc, ticks = (int(v) for v in clk.cpu())
        mhz = 100.0 * cyc / max(ticks, 1)
        fl = 2.0 * cin * cout * frames * hw[0] * hw[1]
        tf = fl / us / 1e6
        out['shapes']['%d->%d' % (cin, cout)] = {
            'flops_per_launch': fl, 'avg_us': round(us, 2), 'tflops': round(tf, 1), 'frac': round(tf / PEAK_F32_TFLOPS, 3),
            'shader_clock_mhz_under_load': round(mhz, 0),
            # the fp32 MFMA rate at the clock the shader really holds: 256 CUs x 4 SIMDs x 64 FLOP per cycle (v_mfma_f32_16x16x4_f32: 2048 FLOP in 32 cycles)
            'frac_of_rate_at_that_clock': round(tf / (256 * 4 * 64 * mhz * 1e6 / 1e12), 3) if mhz > 0 else None,
            'epilogue': 'BN + residual + ReLU' if with_res else 'BN + ReLU'}
        tot_fl += fl
        tot_us += us
    out.update({'flops_per_launch': tot_fl / 2, 'avg_us': round(tot_us / 2, 2), 'tflops': round(tot_fl / tot_us / 1e6, 1),
                'frac': round(tot_fl / tot_us / 1e6 / PEAK_F32_TFLOPS, 3),
                'shader_clock_mhz_under_load': round(sum(v['shader_clock_mhz_under_load'] for v in out['shapes'].values()) / 2, 0),
                'note': 'kernel ALONE (one lane); in the timed region two lanes overlap and fill each other\'s tails (per_launch above). frac = against the data-sheet '
                        'peak (157.3 TFLOP/s at 2.4 GHz); frac_of_rate_at_that_clock = against 256 x 4 x 64 FLOP/cycle at the measured shader clock'})
    # share of the trunk's kernel time: from the newest committed kernel trace of the bench command (profiles/rNN_steady_state.csv)
    import glob as _glob
    for sf in sorted(_glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_steady_state.csv')), reverse=True):
        try:
            for ln in open(sf):
                if ln.startswith(('"void k_conv_igemm<64, 64, 2, 4, 1, 32>', 'k_conv_igemm_p', '"k_conv_igemm_p')):
                    sh = out.setdefault('share_of_steady_state_busy_time', {'percent': 0.0, 'source': 'profiles/' + os.path.basename(sf)})
                    sh['percent'] = round(sh['percent'] + float(ln.rsplit(',', 1)[1]), 2)
            break
        except Exception:      # noqa: BLE001
            pass
    return out


def dataset_specs(n_seq, size=(480, 854), seed=2017):
    """(name, frames, objects, seed) of a DAVIS-2017-val-like synthetic dataset: 1-5 objects (mean ~2.4), 34-104 frames (SURVEY.md 8d config 3;
    the reference's dv2017val has 30 sequences).  Deterministic: every rank derives the same list."""
    import random
    rng = random.Random(seed)
    base = [1] * 8 + [2] * 9 + [3] * 8 + [4] * 2 + [5] * 3
    objs = [base[i % len(base)] for i in range(n_seq)]
    rng.shuffle(objs)
    return [('d%03d' % i, rng.randint(34, 104), objs[i], 500 + i) for i in range(n_seq)]


def build_sequences(specs, size):
    """The synthetic frames of a dataset, generated on the host BEFORE any clock starts (a real dataset lies on disk decoded by the
    loader; generating textures is not part of the metric)."""
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    return [SyntheticSequence(name, L, size, n_obj, seed=seed) for name, L, n_obj, seed in specs]


def run_dataset_shard(tracker, seqs, dev, prefetch=True):
    """The reference's run_dataset loop (model/tracker.py:82-99) over this rank's sequences: sequence.preload(device) + run_sequence per
    sequence.  Returns the per-sequence frames/s as run_sequence reports them (initialize() included, preload not: tracker.py:130,159-161),
    total frames, total seconds of the loop (preloads included) and the update-work counters summed over the sequences."""
    from frtm_vos_amd.lib.datasets import SequencePrefetcher
    fps, frames, agg = [], 0, {}
    run_dataset_shard.enqueue_ms = 0.0
    t0 = time.time()
    # (the reference's sequence.preload(device), tracker.py:91, inside the dataset loop -- here for the NEXT sequence on a copy stream while
    # this one is tracked, exactly as Tracker.run_dataset does it; --no-prefetch: one after the other)
    for seq in SequencePrefetcher(seqs, dev, enabled=prefetch, avoid=getattr(tracker, 'busy_streams', None)):
        out, f = tracker.run_sequence(seq)
        run_dataset_shard.enqueue_ms += 1e3 * getattr(tracker, 'last_enqueue_seconds', 0.0)
        c = path_counters(tracker, seq, len(out))
        for k, v in c.items():
            agg[k] = (agg.get(k, True) and v) if isinstance(v, bool) else agg.get(k, 0) + v
        fps.append(f)
        frames += len(out)
    torch.cuda.synchronize()
    return fps, frames, time.time() - t0, agg


def init_sweep(tracker, size, dev, counts=(1, 2, 5), reps=3):
    """Device time of Tracker.initialize() (augmentation + trunk on the augmented stacks + joint GN/CG fits) for 1 / 2 / 5
    objects starting on frame 0, HIP events, best of `reps` after one untimed call."""
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    out = {}
    # (on the tracker's own stream, like Tracker.run_sequence: the default stream is the legacy null stream, and ANOTHER fresh stream may share a
    #  hardware queue with a trunk lane -- the lanes then run one after the other: +1 ms per initialize(), seen in round 6 when one more stream
    #  of the process moved this leg's stream onto a lane's queue)
    own = getattr(tracker, '_main_stream', None) or torch.cuda.Stream(device=dev)
    own.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(own):
        _init_sweep(tracker, size, dev, counts, reps, out)
    torch.cuda.current_stream().wait_stream(own)
    tracker.release_targets()
    tracker.clear()
    return out


def _init_sweep(tracker, size, dev, counts, reps, out):
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    for n in counts:
        seq = SyntheticSequence('init%d' % n, 1, size, n, seed=40 + n)
        seq.preload(dev)
        im, lb, ids = seq[0]
        best = None
        for r in range(reps + 1):
            tracker.release_targets()
            tracker.clear()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tracker.initialize(im, lb, ids)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            if r > 0:
                best = ms if best is None else min(best, ms)
        out[str(n)] = round(best, 3)


def launch_check(args, rank, world):
    """The N > 1 plumbing of main() without the GPU workload: every rank 'processes' --steps frames in (rank + 1) x 10 ms."""
    import torch.distributed as dist
    from frtm_vos_amd.shard import aggregate_reports, write_rank_report
    used, seen, derr = None, None, None
    if world > 1:
        _, used, seen, _, derr = init_dist('gloo' if args.dist_backend != 'nccl' or not torch.cuda.is_available() else 'nccl', world,
                                           'cuda:0' if torch.cuda.is_available() else None, nccl_timeout_s=90)
        dist.barrier()
    my_frames, mine = args.steps, None
    if args.sequences > 0:                      # sharded mode: this rank's share of the dataset (the same cut main() makes)
        from frtm_vos_amd.shard import shard_indices
        specs = dataset_specs(args.sequences, (480, 854))
        mine = shard_indices(len(specs), rank, world, costs=[L * k for _, L, k, _ in specs])
        my_frames = sum(specs[i][1] for i in mine)
    t0 = time.time()
    time.sleep(0.01 * (rank + 1))
    if world > 1:
        dist.barrier()
    T_rank = T = time.time() - t0
    total = world * my_frames
    if world > 1:
        tt = torch.tensor([T], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        T = float(tt.item())
        if mine is not None:
            ff = torch.tensor([float(my_frames)], dtype=torch.float64)
            dist.all_reduce(ff, op=dist.ReduceOp.SUM)
            total = int(ff.item())
    write_rank_report(args.report_dir, rank, world, dict(frames=my_frames, seconds=T_rank, fps=my_frames / T_rank, launch_check=True,
                                                         sequence_ids=mine))
    if world > 1:
        dist.barrier()
    if rank == 0:
        fps_files, frames, _ = aggregate_reports(args.report_dir, world)
        print(json.dumps({'launch_check': True, 'n_gpus': world, 'steps': args.steps, 'value': total / T, 'unit': 'frames/s',
                          'frames_from_rank_reports': frames, 'frames_total': total, 'scaling': 'weak' if mine is None else 'strong',
                          'dist_backend_used': used, 'rccl_ranks_seen': seen, 'rccl_error': derr}), flush=True)
    if world > 1:
        dist.barrier()
        if derr is None:
            dist.destroy_process_group()
        else:                               # (a failed RCCL group is not torn down collectively: it may never return)
            sys.stdout.flush()
            os._exit(0)


_T0 = time.time()


def _phase(msg):
    """Wall-clock of the bench's own phases, to stderr (the JSON line on stdout stays alone)."""
    print('[bench %6.1f s] %s' % (time.time() - _T0, msg), file=sys.stderr, flush=True)


def main():
    if os.environ.get('FRTM_BENCH_WATCHDOG'):          # debugging aid: dump every thread's Python stack after N seconds and exit
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ['FRTM_BENCH_WATCHDOG']), exit=True)
    args = parse()
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(self_launch(args))
    if args.report_dir is None:
        args.report_dir = default_report_dir()
    rank = int(os.environ.get('RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    local = int(os.environ.get('LOCAL_RANK', 0))
    if world != max(args.gpus, 1):
        sys.exit('bench.py: --gpus %d but WORLD_SIZE=%d (launch with --nproc-per-node equal to --gpus, or let bench.py start the ranks)'
                 % (args.gpus, world))
    if args.share_gpu:
        local = 0
    elif world > 1 and not args.no_pin and not args.launch_check:
        # one process per GPU means ONE GPU per process: the rank sees only its own device, as device 0 -- set before
        # the HIP runtime initialises (nothing has touched the GPU yet).  An existing HIP_VISIBLE_DEVICES list is indexed, not replaced.
        vis = [v for v in os.environ.get('HIP_VISIBLE_DEVICES', '').split(',') if v != '']
        os.environ['HIP_VISIBLE_DEVICES'] = vis[local] if local < len(vis) else str(local)
        local = 0
    if args.launch_check:
        return launch_check(args, rank, world)
    dev = 'cuda:%d' % (local if world > 1 else 0)
    coll, dist_used, rccl_seen, red_dev, dist_err = None, None, None, 'cpu', None
    if world > 1:
        import torch.distributed as dist
        torch.cuda.set_device(local)
        # control group gloo; RCCL on top of it when it comes up on every rank, else gloo for the barrier / max-reduce as well (init_dist)
        coll, dist_used, rccl_seen, red_dev, dist_err = init_dist(args.dist_backend, world, dev)
    else:
        dist = None
        torch.cuda.set_device(0)
    size = tuple(int(v) for v in args.size.split('x'))

    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    from frtm_vos_amd.shard import write_rank_report, pin_host_threads_near_gpu

    # the rank's host threads on cores of its GPU's NUMA node (this GPU's share of them): the thread that enqueues the launches must not
    # be migrated across sockets in the middle of a 46 ms sequence (shard.py: pin_host_threads_near_gpu; --no-cpu-pin)
    if args.no_cpu_pin:
        host_cpus = []
    elif args.share_gpu and world > 1:
        # dress rehearsal (N ranks on ONE GPU): every rank takes its 1/N share of this GPU's cores, as N ranks on N GPUs of a node would
        host_cpus = pin_host_threads_near_gpu(torch.device(dev).index, share=(rank, world))
    else:
        host_cpus = pin_host_threads_near_gpu(torch.device(dev).index)

    params = Parameters(None, fast=args.fast, device=dev, feature_extractor=args.backbone, feature_batch=args.trunk_batch,
                        trunk_lanes=args.trunk_lanes, aug_fill='pull_push' if args.pull_push_fill else 'telea')
    params.disc_params['memory_size'] = args.memory
    params.refiner_factory = lambda chans: synthetic_refiner(args, chans)
    tracker = params.get_model()
    _phase('tracker built')
    if not os.environ.get('FRTM_NO_HOLD_GC'):
        # driver-level (process-global) choices the library no longer makes by itself: long-lived objects into the permanent generation,
        # cyclic collector held off while a sequence's launches are enqueued (a generation-2 collection stops the host for 40-50 ms)
        from frtm_vos_amd.lib.utils import freeze_long_lived_objects
        freeze_long_lived_objects()
        tracker.hold_gc = True
    tracker.prefetch_stream = args.overlap
    tracker.pipeline_passes = args.pipeline
    tracker.balance_batches = args.balance
    if args.no_fold_tail:
        tracker.fold_tail = 0
    tracker.first_batch = args.first_batch or None
    tracker.graph_trunk = args.trunk_graph
    tracker.graph_refiner = bool(args.refiner_graph) and not args.no_refiner_graph
    if args.no_window_inserts:
        from frtm_vos_amd.model.discriminator import Discriminator as _D
        _D.window_inserts = False
    tracker.refiner.parallel_levels = not args.refiner_serial
    tracker.init_lanes = args.init_lanes
    tracker.overlap_first_pass = args.first_pass_overlap
    tracker.early_first_pass = not args.no_early_first_pass
    if args.no_winograd:
        tracker.refiner.use_winograd = False
        tracker.feature_extractor.winograd = False
    if args.no_winograd4:
        tracker.feature_extractor.winograd4 = False
    tracker.window_tracking = not args.no_windows
    if args.init_graph:
        from frtm_vos_amd.model.discriminator import Discriminator
        Discriminator.graph_init = True
    if args.no_persistent_cg or args.share_gpu:         # ranks sharing one GPU would starve each other's resident launches
        from frtm_vos_amd.model.discriminator import Discriminator
        Discriminator.persistent_cg = False
    tracker.eval()
    torch.set_grad_enabled(False)

    timer = StageTimer()
    ext = tracker.feature_extractor
    ext.pass_frames = []
    ext.pass_events = []                     # HIP events around every trunk pass, recorded on the stream the pass runs on
    ext.pass_exec_flops = []                 # executed (Winograd-aware) FLOPs of the same passes
    ext.pass_form_flops = []                 # algorithmic FLOPs of the same passes by kernel form (direct, F(2x2,3x3), F(4x4,3x3))
    aug_log = []
    raw_augment = tracker.augment

    def logged_augment(im, lb):
        out = raw_augment(im, lb)
        aug_log.append(out)                      # references only (no copy inside the timed region)
        return out
    logged_augment.wraps_augmenter = True       # (Tracker.initialize may start the objects' hole fills together: model/augmenter.py: prefetch_fills)
    tracker.augment = timer.wrap('init_augment', logged_augment)
    tracker.augment.wraps_augmenter = True
    tracker.initialize = timer.wrap('initialize_total', tracker.initialize)
    tracker.refiner.forward = timer.wrap('refiner', tracker.refiner.forward)
    tracker.track_window = timer.wrap('track_window', tracker.track_window)          # (contains 'refiner' and 'target_update')
    from frtm_vos_amd.model.discriminator import Discriminator as _Disc
    _Disc.update_window = timer.wrap('target_update', _Disc.update_window)            # window memory inserts + the re-solve at a window's end
    import frtm_vos_amd.model.tracker as _TR
    _TR.TargetObject.initialize = timer.wrap('init_fit', _TR.TargetObject.initialize)

    # Untimed warm-up: a throw-away sequence (other seed) of the SAME length and object count as the timed one, so that every
    # hipGraph the timed frames replay (refiner per window shape; captured at the SECOND use of a shape) exists and the caching allocator holds
    # every block size the timed sequence asks for; preceded by a W-frame sequence when W asks for more than that.
    # The same-length sequence runs TWICE: graphs are captured on the second use of a shape, so only a second pass
    # without captures leaves every block the timed sequence needs in the cache (device_mallocs_in_timed_region must be 0).
    warm_lengths = ([args.warmup] if args.warmup > args.steps else []) + [args.steps, args.steps]
    seq = SyntheticSequence('bench', args.steps, size, args.objects, seed=1 + rank, late_object_at=args.late_object)
    seq.preload(dev)
    for i, wl in enumerate(warm_lengths):
        warm = SyntheticSequence('warm', max(wl, 2), size, args.objects, seed=100 + 7 * i + rank, late_object_at=args.late_object)
        warm.preload(dev)
        run_sequence(tracker, warm)                     # untimed: code objects, allocator growth, trunk arena, graph capture
        _phase('warm-up sequence %d done' % i)
        del warm
    torch.cuda.synchronize()
    timer.reset()
    del aug_log[:]
    del ext.pass_events[:]
    del ext.pass_frames[:]
    del ext.pass_exec_flops[:]
    del ext.pass_form_flops[:]

    repeats = 1 if args.sequences > 0 else max(1, args.repeats)
    shard, shard_seqs, shard_counters, mine = None, None, None, None
    if args.sequences > 0:
        # sharded mode (BASELINE config 4's shape): the dataset is cut over the ranks by cost = frames x objects, longest first
        from frtm_vos_amd.shard import shard_indices
        specs = dataset_specs(args.sequences, size)
        mine = shard_indices(len(specs), rank, world, costs=[L * k for _, L, k, _ in specs])
        shard_seqs = build_sequences([specs[i] for i in mine], size)
        if args.shard_warm:
            run_dataset_shard(tracker, shard_seqs, dev, prefetch=not args.no_prefetch)
            _phase('shard warm pass done')
    # the sequences of the repeats, resident before any clock starts (repeat 0 = the sequence of rounds 1-3: seed 1 + rank)
    rep_seqs = [seq]
    for r in range(1, repeats):
        sq = SyntheticSequence('bench%d' % r, args.steps, size, args.objects, seed=1 + rank + 1000 * r, late_object_at=args.late_object)
        sq.preload(dev)
        rep_seqs.append(sq)
    runs = []
    for rep in range(repeats):
        seq = rep_seqs[rep]
        timer.reset()
        del aug_log[:]
        del ext.pass_events[:]
        del ext.pass_frames[:]
        del ext.pass_exec_flops[:]
        del ext.pass_form_flops[:]
        if dist is not None:
            dist.barrier(group=coll)
        torch.cuda.synchronize()
        # target-model start weights are the reference's: drawn from torch's global CPU generator (the first object of the process from this
        # seed, every later one after initialize()'s manual_seed(0), reference tracker.py:174-180; fixture G15): the CPU leg repeats them
        torch.manual_seed(4242 + rank)
        dev_allocs0 = torch.cuda.memory_stats(dev).get('num_device_alloc', 0)
        if args.debug_allocs:
            torch.cuda.memory._record_memory_history(enabled='all', context='alloc', stacks='python')
        t0 = time.time()
        if shard_seqs is not None:
            seq_fps, n_shard, _, shard_counters = run_dataset_shard(tracker, shard_seqs, dev, prefetch=not args.no_prefetch)
            shard = dict(sequences=len(mine), sequence_ids=mine, mean_of_per_sequence_fps=sum(seq_fps) / max(len(seq_fps), 1))
            outputs = []
        else:
            outputs = run_sequence(tracker, seq)
        torch.cuda.synchronize()
        if args.debug_allocs:
            snap = torch.cuda.memory._snapshot()
            torch.cuda.memory._record_memory_history(enabled=None)
            for tr in snap.get('device_traces', []):
                for ev in tr:
                    if ev.get('action') == 'segment_alloc':
                        frames = [f for f in ev.get('frames', []) if 'site-packages' not in f['filename']][:6]
                        print('hipMalloc of %d bytes on stream %s:' % (ev['size'], ev.get('stream')), file=sys.stderr)
                        for f in frames:
                            print('    %s:%d %s' % (f['filename'], f['line'], f['name']), file=sys.stderr)
        if dist is not None:
            dist.barrier(group=coll)
        T_rank = T = time.time() - t0
        n = len(outputs) if shard is None else n_shard
        n_total = world * n
        mallocs = torch.cuda.memory_stats(dev).get('num_device_alloc', 0) - dev_allocs0
        if dist is not None:
            tt = torch.tensor([T], device=red_dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX, group=coll)
            T = float(tt.item())
            if shard is not None:                       # ranks hold different numbers of frames: sum them
                nn_ = torch.tensor([float(n)], device=red_dev, dtype=torch.float64)
                dist.all_reduce(nn_, op=dist.ReduceOp.SUM, group=coll)
                n_total = int(nn_.item())
        runs.append(dict(seq=seq, outputs=outputs, T=T, T_rank=T_rank, n=n, n_total=n_total, mallocs=mallocs,
                         counters=path_counters(tracker, seq, n) if shard is None else shard_counters,
                         quality=tracking_quality(outputs, seq) if shard is None else float('nan'),
                         tot=timer.totals(), pass_events=list(ext.pass_events), pass_frames=list(ext.pass_frames),
                         exec_flops=list(ext.pass_exec_flops), form_flops=list(ext.pass_form_flops), aug=list(aug_log),
                         enqueue_ms=1e3 * getattr(tracker, 'last_enqueue_seconds', 0.0)))
        _phase('timed repeat %d: %.1f frames/s' % (rep, n_total / T))
    dumped = None
    if args.dump_outputs and rank == 0:
        # the LAST repeat (its sequence is fixed by the arguments; which repeat is the median depends on the clock), its last frame
        dumped = dict(dir=os.path.abspath(args.dump_outputs), repeat=len(runs) - 1, frame=len(runs[-1]['outputs']) - 1,
                      sequence_seed=1 + rank + 1000 * (len(runs) - 1), target_model_seed=4242 + rank)
        dumped['files'] = dump_outputs(args.dump_outputs, {'labels_last_step': runs[-1]['outputs'][-1]})
        _phase('outputs of repeat %(repeat)d, frame %(frame)d (sequence seed %(sequence_seed)d) written to %(dir)s' % dumped)
    # the line reports the MEDIAN repeat (by wall time; every rank holds the same max-reduced times, so every rank picks the same one)
    order = sorted(range(len(runs)), key=lambda i: runs[i]['T'])
    med = runs[order[len(order) // 2]]
    seq, outputs, T, T_rank, n, n_total = med['seq'], med['outputs'], med['T'], med['T_rank'], med['n'], med['n_total']
    mallocs = max(r_['mallocs'] for r_ in runs)
    aug_log = med['aug']
    ext.pass_events, ext.pass_frames, ext.pass_exec_flops, ext.pass_form_flops = med['pass_events'], med['pass_frames'], med['exec_flops'], med['form_flops']

    # ---- what the timed region did ---------------------------------------------------------------------------------
    counters = med['counters']
    quality = med['quality']
    tot = med['tot']
    # trunk passes of the timed region: the time the stream spent in each pass (events recorded after the pass's wait for the
    # previous pass), its algorithmic FLOPs and conv launches.  The first tracking pass runs on a side stream under the host-bound
    # augmentation of initialize(); the other passes are alone on the GPU.
    # (passes may OVERLAP since round 4 -- initialize()'s pass over the augmented stacks runs on the trunk's second lane set next to the
    # first tracking pass -- so the trunk time is the UNION of the pass intervals, measured against the first pass's start event)
    if ext.pass_events:
        ref = ext.pass_events[0][0]
        iv = sorted((ref.elapsed_time(a), ref.elapsed_time(b)) for a, b, _, _ in ext.pass_events)
        bb_ms, cs, ce = 0.0, None, None
        for a_, b_ in iv:
            if ce is None or a_ > ce:
                if ce is not None:
                    bb_ms += ce - cs
                cs, ce = a_, b_
            else:
                ce = max(ce, b_)
        bb_ms += (ce - cs) if ce is not None else 0.0
    else:
        bb_ms = 0.0
    bb_calls = len(ext.pass_events)
    flops_total = sum(f for _, _, f, _ in ext.pass_events)
    n_launch = sum(n for _, _, _, n in ext.pass_events)
    tot['trunk'] = (bb_ms, bb_calls)
    achieved = flops_total / (bb_ms * 1e-3) / 1e12 if bb_ms > 0 else 0.0
    report = dict(counters, frames=n, seconds=T_rank, fps=n / T_rank, mean_iou_vs_synthetic_gt=None if quality != quality else quality,
                  device_mallocs_in_timed_region=mallocs, stage_ms_total={k: round(v[0], 2) for k, v in tot.items()},
                  trunk_tflops=achieved, seed=1 + rank,
                  host_enqueue_ms=round(getattr(run_dataset_shard, 'enqueue_ms', 0.0) if shard is not None else med['enqueue_ms'], 2),
                  host_cpus=('%d-%d (%d)' % (min(host_cpus), max(host_cpus), len(host_cpus))) if host_cpus else 'not pinned',
                  torch_threads=torch.get_num_threads(), sequence_ids=mine)
    if rank == 0:
        from frtm_vos_amd.shard import describe_gpu_numa
        report['gpu_numa_sysfs'] = describe_gpu_numa(torch.device(dev).index)
    write_rank_report(args.report_dir, rank, world, report)
    problems = []
    for ri, cn in enumerate(r_['counters'] for r_ in runs):          # EVERY repeat must have done the scheduled work
        if not cn['all_finite']:
            problems.append('repeat %d: non-finite values in the target models / masks' % ri)
        if cn['cg_persistent_aborts']:
            problems.append('repeat %d: %d persistent CG launches timed out' % (ri, cn['cg_persistent_aborts']))
        if not args.random_refiner:
            if cn['memory_inserts'] + cn['early_outs_fewer_than_10_px'] < cn['memory_inserts_scheduled'] or \
                    cn['memory_inserts'] < cn['memory_inserts_scheduled'] - max(1, 0.1 * cn['memory_inserts_scheduled']):
                problems.append(('repeat %d: ' % ri) + 'memory inserts %(memory_inserts)d of %(memory_inserts_scheduled)d scheduled (%(early_outs_fewer_than_10_px)d early-outs "fewer than 10 pixels")' % cn)
            if cn['cg_solves'] < cn['cg_solves_scheduled'] - cn['early_outs_fewer_than_10_px'] or \
                    cn['cg_solves'] < cn['cg_solves_scheduled'] - max(1, 0.1 * cn['cg_solves_scheduled']):    # (at most 10 % legitimate early-outs, or one)
                problems.append(('repeat %d: ' % ri) + 'filter re-solves %(cg_solves)d of %(cg_solves_scheduled)d scheduled (%(early_outs_fewer_than_10_px)d early-outs "fewer than 10 pixels")' % cn)
    ok = torch.tensor([0.0 if problems else 1.0], device=red_dev)
    if dist is not None:
        dist.all_reduce(ok, op=dist.ReduceOp.MIN, group=coll)
    if problems:
        print('bench.py rank %d: INVALID RUN: %s' % (rank, '; '.join(problems)), file=sys.stderr)

    exec_flops = sum(getattr(ext, 'pass_exec_flops', []) or [0.0])
    exec_ratio = (exec_flops / flops_total) if (flops_total > 0 and exec_flops > 0) else 1.0
    form = [sum(f[k] for f in (getattr(ext, 'pass_form_flops', []) or [[0.0, 0.0, 0.0, 0.0]])) for k in range(4)]
    wino_share = round((form[1] + form[2] + form[3]) / max(sum(form), 1.0), 4)
    wino4_share = round(form[2] / max(sum(form), 1.0), 4)
    wino6_share = round(form[3] / max(sum(form), 1.0), 4)
    sq_busy = None
    import glob as _glob
    for sf in sorted(_glob.glob(os.path.join(ROOT, 'profiles', 'r[0-9][0-9]_sq_busy.json')), reverse=True):      # the NEWEST round's PMC pass first
        try:
            sq_busy = dict(json.load(open(sf))['conv_family'], source='profiles/' + os.path.basename(sf))
            break
        except Exception:      # noqa: BLE001
            sq_busy = None
    traffic = None
    tf = os.path.join(ROOT, 'profiles', 'pmc_traffic.json')      # written by tools/pmc_summary.py from the rocprofv3 --pmc passes
    if os.path.exists(tf):
        try:
            traffic = json.load(open(tf))['conv_family']['bytes_per_launch']
        except Exception:
            traffic = None
    out = {
        'metric': 'segmented frames/sec/GPU (480p, ResNet101, full CG iters)',
        'value': n_total / T, 'unit': 'frames/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
        # `warmup` echoes --warmup (the contract's W).  What really ran untimed is MORE: whole throw-away sequences of the timed length, twice (graphs
        # are captured at the second use of a shape, and only a capture-free pass leaves the allocator warm), plus a W-frame one when W > steps
        'warmup_frames_run': sum(max(w, 2) for w in warm_lengths),
        'ms_per_step': 1e3 * T * world / max(n_total, 1), 'higher_is_better': True, 'scaling': 'weak' if shard is None else 'strong', 'vs_baseline': None,
        'dtype': 'f32', 'data': 'synthetic',
        'config': {'workload': ('' if shard is None else '%d dv2017val-like synthetic sequences (1-5 objects, 34-104 frames) SHARDED over the ranks by frames x objects; per sequence as in: ' % args.sequences) +
                               'dv2017val-like synthetic sequence per GPU: %s, %dx%d, %d objects, %d frames incl. initialize(), '
                               '%s iterations, memory %d, c=96, synthetic weights (trunk: seeded random, residual-branch BN x0.25; refiner: %s), '
                               'first-frame hole fill %s, trunk fed %d frames per pass in %d concurrent lanes, '
                               'frames between two filter re-solves tracked as one window%s, 3x3 stride-1 convs %s (fp32)' %
                               (args.backbone, size[0], size[1], args.objects, args.steps,
                                'fast (5,10,10,10)/(5,)' if args.fast else 'full (5,10,10,10,10)/(10,)', args.memory,
                                'seeded default init, no confident masks' if args.random_refiner else 'seeded default init + score-following channel',
                                'pull-push on the device' if args.pull_push_fill else "Telea on the host (the reference's recipe restated)",
                                args.trunk_batch, args.trunk_lanes,
                                ' (off)' if args.no_windows else '', 'direct' if args.no_winograd else ('Winograd F(2x2,3x3)' if args.no_winograd4 else 'Winograd F(6x6,3x3) / F(4x4,3x3) from 128 channels on, F(2x2,3x3) below')),
                   'parallelism': 'one process per GPU, sequences sharded, no collectives on the data path'},
        'roofline': {'bound': 'mfma', 'kernel': 'k_conv_igemm / k_conv3x3_halo / k_conv3x3_wino / k_wino4_* (fp32 MFMA convs of the whole ResNet trunk; FLOPs counted in direct form)',
                     'achieved': achieved, 'peak': PEAK_F32_TFLOPS, 'unit': 'TFLOP/s', 'frac': achieved / PEAK_F32_TFLOPS,
                     # `frac` counts ALGORITHMIC (direct-form) FLOPs.  The 3x3 stride-1 convs of large launches run as Winograd F(2x2,3x3)
                     # (16 instead of 36 multiplications per 2x2 outputs) or, from 128 channels on, F(4x4,3x3) / F(6x6,3x3) (36 instead of 144 per 4x4
                     # outputs, 64 instead of 324 per 6x6), so the MACs the matrix pipes EXECUTE are fewer.  frac_executed
                     # counts those (frtm_backbone_last_flops_executed); mfma_pipe_busy is the SQ counter ratio of the committed PMC pass
                     # over the same kernels (profiles/*_sq_busy.json: SQ_VALU_MFMA_BUSY_CYCLES / active cycles, every kernel alone).
                     'achieved_executed': achieved * exec_ratio, 'frac_executed': achieved * exec_ratio / PEAK_F32_TFLOPS,
                     'winograd_share_of_algorithmic_flops': wino_share, 'winograd_f4x4_share_of_algorithmic_flops': wino4_share,
                     'winograd_f6x6_share_of_algorithmic_flops': wino6_share,
                     'mfma_pipe_busy': sq_busy,
                     # v_mfma_f32_16x16x4_f32 (the instruction of these kernels) alone in a loop of eight MFMAs and a wait sustains 151-153 TFLOP/s
                     # (round 5's probe, tools/mfma_valu_probe.hip, profiles/r05_mfma_valu_probe.txt; round 3's loop form reached 139.8): there is
                     # no issue bubble inherent to the instruction, `peak` stays the data-sheet number
                     'instruction_ceiling_16x16x4': {'tflops': 152.0, 'source': 'profiles/r05_mfma_valu_probe.txt'},
                     'traffic': traffic,
                     # avg_ms = HIP-event time of the trunk passes / conv launches: the EFFECTIVE duration per launch.  With
                     # trunk_lanes concurrent sub-batches the kernel-trace mean duration is ~lanes x this (kernels share the GPU);
                     # profiles/*_trunk_only.json holds the union-of-intervals cross-check from rocprofv3.
                     'per_launch': {'flops': flops_total / max(n_launch, 1), 'avg_ms': bb_ms / max(n_launch, 1), 'launches': n_launch,
                                    'concurrent_lanes': args.trunk_lanes},
                     'trunk_ms_per_pass': bb_ms / max(bb_calls, 1),
                     # every pass of the timed region in order: [frames, ms, TFLOP/s] (the augmented first-frame stack, then the
                     # tracking passes; the first tracking pass is enqueued before initialize() and shares the GPU with it)
                     'passes': [[nf, round(a.elapsed_time(b), 3), round(f / a.elapsed_time(b) / 1e9, 1)]
                                for (a, b, f, _), nf in zip(ext.pass_events, ext.pass_frames)],
                     # the same passes as [start, end] in ms after the first pass's start (they overlap where the second lane set is used)
                     'pass_intervals_ms': [[round(ext.pass_events[0][0].elapsed_time(a), 3), round(ext.pass_events[0][0].elapsed_time(b), 3)]
                                           for a, b, _, _ in ext.pass_events] if ext.pass_events else []},
        'stage_ms_total': {k: round(v[0], 2) for k, v in tot.items()},
        # event spans on the tracker's stream.  Since the streams are placed on hardware queues of their own (stream_placement below)
        # initialize()'s augmentation RUNS UNDER the first tracking pass and its own trunk call then waits for that pass: 'initialize_total'
        # spans the first tracking pass as well (what initialize() costs on its own is initialize_ms_by_objects)
        'stage_ms_note': 'initialize_total overlaps the first tracking pass (trunk) when stream_placement.first.independent',
        'path_counters': counters,
        'mean_iou_vs_synthetic_gt': None if quality != quality else round(quality, 4),
        'device_mallocs_in_timed_region': mallocs,
        # wall-clock until the host had enqueued the whole sequence (run_sequence, before its final synchronise)
        'host_enqueue_ms_total': round(med['enqueue_ms'], 2),
        # the headline as a distribution: `value` is the MEDIAN of `repeats` fresh sequences (each K frames, each bracketed by barrier +
        # synchronize; max over ranks per repeat), in run order below; a slow-cluster run (host stall) shows up as min << median
        'repeats': {'n': len(runs), 'value_is': 'median', 'values_fps': [round(r_['n_total'] / r_['T'], 1) for r_ in runs],
                    'min_fps': round(min(r_['n_total'] / r_['T'] for r_ in runs), 1), 'max_fps': round(max(r_['n_total'] / r_['T'] for r_ in runs), 1),
                    'host_enqueue_ms_per_sequence': [round(r_['enqueue_ms'], 2) for r_ in runs],
                    'mean_iou_vs_synthetic_gt': [None if r_['quality'] != r_['quality'] else round(r_['quality'], 4) for r_ in runs]},
        'host_cpus': ('%d-%d (%d logical CPUs on the NUMA node of the GPU)' % (min(host_cpus), max(host_cpus), len(host_cpus))) if host_cpus else 'not pinned',
        'stream_placement': __import__('frtm_vos_amd.model.tracker', fromlist=['STREAM_PROBE']).STREAM_PROBE,
        'valid': bool(ok.item() > 0),
    }
    if dumped is not None:
        out['dump_outputs'] = dumped           # which repeat / frame the files hold, so that two builds compare the same step
    if world > 1:
        # the group that carried barrier + max-reduce: 'nccl' (= RCCL) or, when RCCL did not come up on every rank with one visible device each, 'gloo'
        out['dist_backend_used'] = dist_used
        out['rccl_ranks_seen'] = rccl_seen
        if dist_err:
            out['rccl_error'] = dist_err
    if shard is not None:
        out['shard_rank0'] = shard
        out['frames_total'] = n_total
    _phase('timed sequence and checks done')
    if args.full and rank == 0 and world == 1:
        aug_cpu = [(a.cpu(), b.cpu()) for a, b in aug_log]
        # The legs below ADD to the line; the headline above is complete without them.  One of them failing (a fixture missing, the host out
        # of memory for the evaluation pool, ...) is reported in the line under "leg_errors" instead of costing the driver the whole line.
        leg_errors = {}

        def leg(name, fn):
            try:
                fn()
            except Exception as ex:      # noqa: BLE001
                import traceback
                leg_errors[name] = '%s: %s' % (type(ex).__name__, ex)
                sys.stderr.write('[bench] leg %s failed:\n%s\n' % (name, traceback.format_exc()))
            _phase('%s done' % name)

        def leg_init_sweep():
            counts = tuple(int(v) for v in args.init_sweep_counts.split(','))
            out['initialize_ms_by_objects'] = init_sweep(tracker, size, dev, counts=counts)
            # the same with the OTHER first-frame hole fill: Telea's method is a host step of ~3 ms per object that a caller of initialize() waits
            # for (run_sequence hides it under the first tracking pass); the pull-push pyramid runs on the device
            aug = tracker.augmenter
            fill0 = aug.fill
            aug.fill = 'pull_push' if fill0 == 'telea' else 'telea'
            try:
                out['initialize_ms_by_objects_%s_fill' % aug.fill] = init_sweep(tracker, size, dev, counts=counts)
            finally:
                aug.fill = fill0
            out['first_frame_hole_fill'] = fill0

        def leg_dataset():
            # the headline above is ONE sequence; this is the dataset-level figure the reference's run_dataset prints (mean of the per-
            # sequence frames/s, model/tracker.py:94,101) over 30 dv2017-like sequences through the same tracker, first-use costs of new
            # shapes included, with the same counters of the update work
            fps_l, fr, sec, cnt = run_dataset_shard(tracker, build_sequences(dataset_specs(30, size), size), dev, prefetch=not args.no_prefetch)
            out['dataset_sim'] = {'sequences': len(fps_l), 'frames': fr, 'mean_of_per_sequence_fps': round(sum(fps_l) / len(fps_l), 1),
                                  'total_fps': round(fr / sec, 1), 'min_sequence_fps': round(min(fps_l), 1), 'max_sequence_fps': round(max(fps_l), 1),
                                  'path_counters': cnt,
                                  'note': '30 synthetic dv2017val-like sequences (1-5 objects, mean 2.4; 34-104 frames; 480x854); total_fps = frames / wall of the loop incl. the host->device preload of every sequence (pageable memory; %s) and the counter read-backs; mean_of_per_sequence_fps is what the reference prints' % ('one after the other' if args.no_prefetch else 'the next sequence on a copy stream while this one is tracked, lib/datasets.py: SequencePrefetcher')}

        def leg_streaming():
            out['streaming'] = streaming_leg(tracker, seq, dev)
            out['streaming_fps'] = out['streaming']['streaming_fps']

        def leg_cg():
            out['roofline_cg'] = cg_roofline(dev, size)
            mk = cg_roofline(dev, size, persistent=False)
            out['roofline_cg']['multi_kernel_form_ms_per_run'] = mk['ms_per_run']

        def leg_dominant():
            out['roofline']['dominant_kernel'] = dominant_kernel_leg(dev)

        def leg_cpu():
            seq.preload('cpu')
            out['cpu_baseline'] = cpu_baseline(args, size, seq, aug_cpu, min(args.cpu_frames, args.steps - 1), gpu_labels=outputs)

        def leg_jf():
            # the DATASET-level parity statement (77 objects) next to the 13-frame sample above
            out.setdefault('cpu_baseline', {})['jf_parity_dataset_level'] = jf_vs_fixture(dev, args.jf_draws)

        if not args.no_init_sweep:
            leg('init sweep', leg_init_sweep)
        if not args.no_dataset_sim and shard is None:
            leg('dataset leg', leg_dataset)
        if not args.no_streaming and shard is None:
            leg('streaming leg', leg_streaming)
        if not args.no_cg_roofline:
            leg('cg roofline', leg_cg)
            if args.backbone == 'resnet101':
                leg('dominant kernel', leg_dominant)
        if not args.no_cpu_baseline and args.late_object is None:
            leg('cpu baseline', leg_cpu)
            if not args.no_jf_fixture and args.backbone == 'resnet101' and os.path.exists(os.path.join(ROOT, 'tests', 'golden', 'g14_jf_float32.npz')):
                leg('dataset-level J&F vs fixture G14', leg_jf)
        if leg_errors:
            out['leg_errors'] = leg_errors
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()                      # (gloo: every rank has reported)
        if dist_err is None:
            dist.destroy_process_group()
        else:                               # an RCCL group that failed to come up is not torn down collectively (it may never return): leave
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(0 if out['valid'] else 3)
    if not out['valid']:
        sys.exit(3)


if __name__ == '__main__':
    main()
