"""The bf16x1 refiner mode (FRTM_WLAYOUT_BF16X1_3X3, Parameters(refiner_precision='bf16x1')) against the fp32 refiner: kernel times of the refiner's
3x3 conv shapes (those of profiles/r05_wino_bench.txt, with and without a residual) on the fp32 form the refiner launches today against the bf16 direct
form per tile form, the bytes-over-bandwidth floor of each launch, the 8-frame x 2-object refiner window, tracker frames/s (Tracker.run_sequence and
frame-by-frame track()), the dataset-level J&F shift on the sequences of fixture G14 and how far the window's logits move.
Writes profiles/bf16x1_refiner_time.txt.

Operands are random (ReLU'd normal activations, normal weights scaled by 1/sqrt(9 Cin)): the clock drops on random data, and zeros or constants
would flatter both arms.  The arms alternate in one process; frtm_clock_probe reports the shader clock under each arm's load.  The routing rule of
ops.bf16x1_3x3_launch (BF16X1_3X3_ROUTES) is read off the per-shape table: a (Cin, Cout) pair is routed only where, on EVERY measured launch of that
pair with at least as many blocks (wino_launch's count), the bf16 median (automatic tile form) beats the fp32 median by more than the spread
(max - min) of the fp32 arm's own per-round figures; the table holds, per pair, the block count of the smallest such launch.
    python tools/refiner_bf16_time.py [--quick] [--no-tracker] [--no-jf] [--route-all]
--route-all: the window / tracker / J&F stages route every 3x3 launch that wino_launch accepts (bf16_min_blocks = 512) instead of the compiled rule."""
import copy
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd import _hip as H, ops  # noqa: E402

DEV = 'cuda:0'
QUICK = '--quick' in sys.argv
MIN_BLOCKS = ops.WINO_MIN_BLOCKS if '--route-all' in sys.argv else None
OUT = os.path.join(ROOT, 'profiles', 'bf16x1_refiner_time.txt')
HBM_TBS = 8.0                 # MI355X peak HBM bandwidth, TB/s: the floor below is bytes / this
lines = []
# (maps, Cin, Cout, H, W) of profiles/r05_wino_bench.txt at 16 maps (an 8-frame window with 2 objects; the base conv runs on the 8 frames).
# The launches of a single frame (frame-by-frame track()) are not in the table: they are routed by the block counts alone.
SHAPES = [(16, 64, 64, 120, 214), (16, 65, 65, 120, 214), (16, 65, 64, 120, 214), (8, 64, 65, 120, 214), (16, 64, 32, 240, 428),
          (16, 64, 64, 60, 107), (16, 65, 65, 60, 107), (16, 64, 64, 30, 54)]


def say(s):
    """Prints a line and keeps the profile on disk up to date (a later stage that fails leaves the earlier ones recorded)."""
    print(s, flush=True)
    lines.append(s)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def clock_under(fn, n):
    """MHz of the shader clock while fn() runs n times (frtm_clock_probe on a side stream)."""
    side = torch.cuda.Stream()
    clk = torch.zeros(2, dtype=torch.int64, device=DEV)
    for _ in range(3):
        fn()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        H.lib().frtm_clock_probe(1000, ctypes.c_void_p(clk.data_ptr()), ctypes.c_void_p(side.cuda_stream))
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    c = clk.cpu()
    return float(c[0]) / max(float(c[1]), 1.0) * 100.0


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / n


def ab(fns, n, rounds):
    """Alternating rounds of the arms; per arm (median, max - min) of its per-round us per call."""
    t = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, n))
    return [(statistics.median(v), max(v) - min(v)) for v in t]


def shape_table():
    g = torch.Generator().manual_seed(0)
    say('%-30s %8s %6s %8s %8s %8s %9s %9s  %-24s %10s %10s' % ('shape', 'fp32 us', '+-', 't1 us', 't2 us', 'floor us', 'fp32/auto', 'MHz f/b',
                                                                'fp32 kernel', 'rms e f32', 'rms e b1'))
    verdict = {}
    for n, cin, cout, hh, ww in SHAPES:
        x = torch.relu(torch.randn(n, cin, hh, ww, generator=g)).to(DEV)
        w = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).to(DEV)
        sc, sh = (torch.rand(cout, generator=g) + 0.5).to(DEV), (torch.randn(cout, generator=g) * 0.1).to(DEV)
        wino = ops.wino_launch(n, hh, ww, cout)                  # the form the fp32 refiner launches for this shape
        wT, kt, lay = ops.pack_weights(w, wino=True) if wino else ops.pack_weights(w)
        wB, _, layB = ops.pack_weights(w, bf16x1=True)
        for with_res in (False, True):
            res = torch.randn(n, cout, hh, ww, generator=g).to(DEV) if with_res else None
            y32 = torch.empty(n, cout, hh, ww, device=DEV)
            yb = torch.empty_like(y32)
            if wino:
                f32 = lambda: ops.conv2d(x, wT, cout, 3, 1, 1, scale=sc, shift=sh, residual=res, relu=True, out=y32, splitk=1, w_layout=2)  # noqa: E731
            else:
                f32 = lambda: ops.conv2d(x, wT, cout, 3, 1, 1, ktab=kt, scale=sc, shift=sh, residual=res, relu=True, out=y32, w_layout=lay)  # noqa: E731

            def fb(tile):
                return lambda: ops.conv2d(x, wB, cout, 3, 1, 1, scale=sc, shift=sh, residual=res, relu=True, out=yb, splitk=1, w_layout=layB, tile=tile)
            f32()
            k32 = H.lib().frtm_conv_last_kernels().decode()
            fb(0)()
            auto = 2 if '<3>' in H.lib().frtm_conv_last_kernels().decode() else 1
            flop = 2.0 * 9 * cin * cout * n * hh * ww
            reps = max(5, int(2e4 / max(1.0, flop / 1e9)))
            if QUICK:
                reps = max(3, reps // 4)
            (t32, sp32), (tb1, _), (tb2, _) = ab([f32, fb(1), fb(2)], reps, 3 if QUICK else 7)
            tauto = tb1 if auto == 1 else tb2
            mhz32, mhzb = clock_under(f32, reps), clock_under(fb(auto), reps)
            floor = (4.0 * n * hh * ww * (cin + cout * (2 if with_res else 1)) + 2.0 * 9 * cin * cout) / (HBM_TBS * 1e12) * 1e6
            if not with_res:
                ref = torch.nn.functional.conv2d(x[:2].double(), w.double(), padding=1) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)
                ref = torch.relu(ref)
                e32 = float((y32[:2].double() - ref).pow(2).mean().sqrt())
                eb = float((yb[:2].double() - ref).pow(2).mean().sqrt())
                del ref
            else:
                e32 = eb = float('nan')                     # (errors are taken on the rows without a residual)
            say('%-30s %8.1f %6.1f %7.1f%s %7.1f%s %8.1f %9.2f %4.0f/%4.0f  %-24s %10.3e %10.3e' % (
                '%2d x %d->%d @ %dx%d%s' % (n, cin, cout, hh, ww, ' +res' if with_res else ''), t32, sp32, tb1, '*' if auto == 1 else ' ', tb2,
                '*' if auto == 2 else ' ', floor, t32 / tauto, mhz32, mhzb, k32.split()[0], e32, eb))
            blocks = n * ((hh + 7) // 8) * ((ww + 7) // 8) * ((cout + 31) // 32)
            verdict.setdefault((cin, cout), []).append((t32 - tauto > sp32, blocks, '%d x %d->%d @ %dx%d%s: %s (fp32 %.1f +- %.1f, bf16x1 automatic form %.1f)' % (
                n, cin, cout, hh, ww, ' +res' if with_res else '', 'FASTER' if t32 - tauto > sp32 else 'not faster', t32, sp32, tauto)))
        del x, w, res, y32, yb
    say('# routing verdicts: faster = fp32 median - bf16x1 median (automatic form) > the fp32 arm\'s spread; a (Cin, Cout) pair is routed from the')
    say('# block count (wino_launch\'s: maps x 8x8 output blocks x 32-channel tiles) of its smallest measured launch from which every measured launch is faster')
    table = {}
    for pair, vs in verdict.items():
        for _, blocks, text in vs:
            say('#   %s [%d blocks]' % (text, blocks))
        losing = [b for won, b, _ in vs if not won]
        winning = [b for won, b, _ in vs if won and b > max(losing, default=-1)]
        if winning:
            table[pair] = min(winning)
    say('# (Cin, Cout) -> fewest blocks to route, from this table: %s' % (dict(sorted(table.items())) or 'none'))
    say('# compiled rule (ops.BF16X1_3X3_ROUTES):                  %s' % (dict(sorted(ops.BF16X1_3X3_ROUTES.items())) or 'none'))


def window():
    """The 8-frame x 2-object refiner window, eager (side stream for the deep levels as in the tracker), both modes; how far the logits move."""
    import oracle.make_golden_jf as JF
    g = torch.Generator().manual_seed(1)
    net = JF.refiner_for('resnet101').to(DEV).eval()
    net.bf16_min_blocks = MIN_BLOCKS
    sizes = {'layer5': (15, 27), 'layer4': (30, 54), 'layer3': (60, 107), 'layer2': (120, 214)}
    feats = {L: torch.relu(torch.randn(8, net.ft_channels[L], *sizes[L], generator=g)).to(DEV) for L in net.ft_channels}
    scores = torch.randn(16, 1, 30, 54, generator=g).to(DEV)
    out, t = {}, {'fp32': [], 'bf16x1': []}
    routed = 0
    for _ in range(3 if QUICK else 7):
        for mode in ('fp32', 'bf16x1'):
            net.precision = mode
            n0 = H.lib().frtm_conv_bf16x1_3x3_launches()
            out[mode] = net(scores, feats, (480, 854)).clone()
            if mode == 'bf16x1':
                routed = H.lib().frtm_conv_bf16x1_3x3_launches() - n0
            t[mode].append(timed(lambda: net(scores, feats, (480, 854)), 5 if QUICK else 20))
    a, b = statistics.median(t['fp32']), statistics.median(t['bf16x1'])
    f, q = out['fp32'].double(), out['bf16x1'].double()
    rng = float(f.max() - f.min())
    say('Refiner window, 8 frames x 2 objects at 480x854 (score-following refiner of fixture G14, random taps), eager: fp32 %.0f us (+- %.0f), bf16x1 %.0f us '
        '(%.3fx); %d of 29 3x3 convs routed per pass' % (a, max(t['fp32']) - min(t['fp32']), b, a / b, routed))
    say('  logits: range %.3f; bf16x1 - fp32 rms %.3e (%.2e of the range), max %.3e (%.2e of the range); label (logit > 0) agreement %.6f' % (
        rng, float((q - f).pow(2).mean().sqrt()), float((q - f).pow(2).mean().sqrt()) / rng, float((q - f).abs().max()), float((q - f).abs().max()) / rng,
        float(((q > 0) == (f > 0)).double().mean())))


def tracker_fps():
    """Frames/s at the headline configuration (ResNet-101, 480x854, 2 objects) per refiner precision, alternating: Tracker.run_sequence (windows,
    batched trunk) and Tracker.track() frame by frame (bench.py: streaming_leg)."""
    import oracle.make_golden_jf as JF
    from oracle.tracker_ref import shift_flip_augment
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    n_frames = 24 if QUICK else 48
    seq = SyntheticSequence('bf16x1r', n_frames, (480, 854), 2, seed=7)
    seq.preload(DEV)
    modes = ('fp32', 'bf16x1')
    trk = {}
    for mode in modes:
        params = Parameters(None, device=DEV, feature_extractor='resnet101', refiner_precision=mode)
        refiner = JF.refiner_for('resnet101')
        params.refiner_factory = lambda chans, r=refiner: copy.deepcopy(r)
        params.disc_params.update(**JF.DISC)
        trk[mode] = params.get_model().eval()
        trk[mode].refiner.bf16_min_blocks = MIN_BLOCKS
        trk[mode].augment = shift_flip_augment
        trk[mode].start_weights = lambda oid: JF.start_weights(7, oid)
        trk[mode].run_sequence(seq)                 # warm-up: graphs captured, workspaces grown
    fps = {m: [] for m in modes}
    routed = 0
    for _ in range(2 if QUICK else 3):
        for mode in modes:
            torch.cuda.synchronize()
            n0 = H.lib().frtm_conv_bf16x1_3x3_launches()
            t0 = time.time()
            trk[mode].run_sequence(seq)
            torch.cuda.synchronize()
            fps[mode].append(n_frames / (time.time() - t0))
            if mode == 'bf16x1':
                routed = H.lib().frtm_conv_bf16x1_3x3_launches() - n0
    a, b = statistics.median(fps['fp32']), statistics.median(fps['bf16x1'])
    say('Tracker.run_sequence, ResNet-101, 480x854, 2 objects, %d frames (first-frame fit included), median of alternating runs: fp32 %.1f frames/s '
        '(runs %s), bf16x1 refiner %.1f frames/s (runs %s; %.3fx); %d bf16x1 3x3 launches per bf16x1 run' % (
            n_frames, a, ' '.join('%.1f' % v for v in fps['fp32']), b, ' '.join('%.1f' % v for v in fps['bf16x1']), b / a, routed))
    sfps = {m: [] for m in modes}
    own = torch.cuda.Stream(device=DEV)
    frames = [seq[t][0] for t in range(len(seq.images))]
    for rnd in range(3 if QUICK else 4):               # round 0 warms up
        for mode in modes:
            t = trk[mode]
            t.release_targets()
            t.clear()
            with torch.cuda.stream(own):
                im, lb, ids = seq[0]
                t.current_frame = 0
                t.initialize(im, lb, ids)
                t.current_frame = 1
                torch.cuda.synchronize()
                t0 = time.time()
                for im in frames[1:]:
                    t.track(im)
                    t.current_frame += 1
                own.synchronize()
                if rnd:
                    sfps[mode].append((len(frames) - 1) / (time.time() - t0))
            torch.cuda.current_stream().wait_stream(own)
            t.release_targets()
            t.clear()
    a, b = statistics.median(sfps['fp32']), statistics.median(sfps['bf16x1'])
    say('Tracker.track() frame by frame, %d frames: fp32 %.1f frames/s (runs %s), bf16x1 refiner %.1f frames/s (runs %s; %.3fx)' % (
        len(frames) - 1, a, ' '.join('%.1f' % v for v in sfps['fp32']), b, ' '.join('%.1f' % v for v in sfps['bf16x1']), b / a))
    seq.release()
    del trk
    torch.cuda.empty_cache()


def jf_shift():
    """Dataset-level J&F of the HIP path on the sequences of fixture G14 (tests/test_north_star_gpu.py: _dataset_jf) with an fp32 and a bf16x1 refiner."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_north_star_gpu as NS
    make = NS._hip_tracker
    res = {}
    try:
        for mode in ('fp32', 'bf16x1'):
            def patched(*a, _mode=mode, **kw):
                trk = make(*a, **kw)
                trk.refiner.precision = _mode
                trk.refiner.bf16_min_blocks = MIN_BLOCKS
                return trk
            NS._hip_tracker = patched
            n0 = H.lib().frtm_conv_bf16x1_3x3_launches()
            hip, ora, agree, n_seq = NS._dataset_jf('g14_jf_float32.npz', 'v2', 'jg%02d', (0,))
            res[mode] = (100 * float(hip.mean()), 100 * float(ora.mean()), agree, n_seq, hip.shape[0], H.lib().frtm_conv_bf16x1_3x3_launches() - n0)
    finally:
        NS._hip_tracker = make
    f, b = res['fp32'], res['bf16x1']
    say('J&F on the %d sequences (%d objects) of fixture G14, one run each: fp32 HIP path %.3f, bf16x1 refiner %.3f (shift %+.3f); recorded oracle %.3f; '
        'label agreement with the oracle fp32 %.5f, bf16x1 %.5f; %d bf16x1 3x3 launches in the bf16x1 run.  '
        'The oracle\'s own single-run sigma: 0.064-0.067 (README)' % (f[3], f[4], f[0], b[0], b[0] - f[0], f[1], f[2], b[2], b[5]))


def main():
    torch.set_grad_enabled(False)
    say('# bf16x1 refiner mode (csrc/conv3x3_bf16x1.hip, v_mfma_f32_32x32x16_bf16) against the fp32 refiner on MI355X: %s' % time.strftime('%Y-%m-%d'))
    say('# operands: ReLU\'d normal activations, normal weights / sqrt(9 Cin); every arm runs scale / shift, ReLU and the residual where marked;')
    say('# us = median of alternating rounds; +-: max - min of the fp32 arm\'s per-round figures; fp32 = the form the refiner launches today (Winograd')
    say('# F(2x2,3x3) where wino_launch accepts the launch); t1 / t2: bf16 tile forms of 64 / 96 output channels (* = the automatic choice);')
    say('# floor: (fp32 activations in + out + residual + bf16 weights) / %.0f TB/s; rms e: against an fp64 conv on the first two maps' % HBM_TBS)
    say('# stages below the table route %s' % ('every 3x3 launch that wino_launch accepts (--route-all)' if MIN_BLOCKS is not None else 'by the compiled rule'))
    shape_table()
    window()
    if '--no-tracker' not in sys.argv:
        tracker_fps()
    else:
        say('Tracker frames/s: not measured in this run')
    if '--no-jf' not in sys.argv:
        jf_shift()
    else:
        say('J&F shift: not measured in this run')
    print('wrote', OUT)


if __name__ == '__main__':
    main()
