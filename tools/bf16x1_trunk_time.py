"""The bf16x1 trunk mode (FRTM_WLAYOUT_BF16X1, Parameters(trunk_precision='bf16x1')) against the fp32 trunk: kernel times of the stride-1 1x1 conv
shapes per tile form, their error against fp64, the bytes-over-bandwidth floor of each launch, whole ResNet-101 trunk passes, tracker frames/s
(Tracker.run_sequence and frame-by-frame track()) and the dataset-level J&F shift on the sequences of fixture G14.
Writes profiles/bf16x1_trunk_time.txt.

Operands are trunk activations of synthetic 480x854 frames (the clock drops on random data): the taps of a seeded ResNet-101 pass, through the
conv1 + BN + ReLU of the next block of that stage for the narrow inputs; weights are that block's conv3 (BN folded); the conv1 shapes (N -> N / 4)
run on the tap itself.  The arms alternate in
one process; frtm_clock_probe reports the shader clock under each arm's load.  The routing rule of csrc/trunk_route.h (kTrunkRules) is read off
the per-shape table: a shape is routed only where the bf16x1 median (automatic tile form) beats the fp32 median by more than the spread (max - min)
of the fp32 arm's own per-round figures in this run.
    python tools/bf16x1_trunk_time.py [--quick] [--no-tracker] [--no-jf]
    python tools/bf16x1_trunk_time.py --oracle-only        (appends the trunk-against-oracle lines to the existing profile)"""
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
from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor  # noqa: E402

DEV = 'cuda:0'
QUICK = '--quick' in sys.argv
OUT = os.path.join(ROOT, 'profiles', 'bf16x1_trunk_time.txt')
HBM_TBS = 8.0                 # MI355X peak HBM bandwidth, TB/s: the floor below is bytes / this
lines = []


def say(s):
    """Prints a line and keeps the profile on disk up to date (a later stage that fails leaves the earlier ones recorded)."""
    print(s, flush=True)
    lines.append(s)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')


def folded(cv, bn):
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).float()
    return cv.weight.data.float(), scale, (bn.bias - bn.running_mean * scale).float()


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


def trunk_vs_oracle():
    """Taps of a ResNet-101 pass against the CPU oracle (oracle/cpu_ref.py), fp32 and bf16x1, as tests/test_bf16x3_gpu.py: test_trunk_vs_oracle
    prints them for bf16x3: max |tap - oracle| / max |oracle| per tap.  Recorded, not gated: the mode is defined by its arithmetic."""
    from oracle import cpu_ref as O
    P = O.resnet_random_params('resnet101', seed=3)
    img = torch.randint(0, 256, (8, 3, 480, 854), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
    ref = O.resnet_forward('resnet101', P, img)
    ext = ResnetFeatureExtractor('resnet101', weights=P).to(DEV)
    ext.lanes = 1

    def rel(a, b):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        return float((a - b).abs().max() / (b.abs().max() + 1e-30))
    say('# ResNet-101 taps against the CPU oracle (seeded weights, 480x854), max |tap - oracle| / max |oracle|, fp32 / bf16x1; one lane, routing as compiled')
    for B in (8, 1):
        out = {}
        for mode in ('fp32', 'bf16x1'):
            ext.precision = mode
            out[mode] = {k: v.cpu() for k, v in ext(img[:B].to(DEV)).items()}
        say('B=%d: %s' % (B, '  '.join('%s %.2e / %.2e' % (k, rel(out['fp32'][k], ref[k][:B]), rel(out['bf16x1'][k], ref[k][:B])) for k in sorted(ref))))
    del ext
    torch.cuda.empty_cache()


def main():
    torch.set_grad_enabled(False)
    if '--oracle-only' in sys.argv:
        lines.extend(open(OUT).read().rstrip('\n').split('\n'))
        trunk_vs_oracle()
        return
    g = torch.Generator().manual_seed(0)
    ext = ResnetFeatureExtractor('resnet101', seed=0).to(DEV)
    ext.lanes = 2
    R = ext.resnet
    img8 = torch.randint(0, 256, (8, 3, 480, 854), dtype=torch.uint8, generator=g).to(DEV)
    taps = ext(img8)
    say('# bf16x1 trunk mode (csrc/conv_bf16x1.hip) against the fp32 trunk on MI355X: %s' % time.strftime('%Y-%m-%d'))
    say('# operands: taps of a seeded ResNet-101 pass on 8 synthetic 480x854 frames; narrow inputs = relu(bn(conv1 of block 1)) of the tap')
    say('# every arm runs the trunk\'s epilogue (BN scale / shift, ReLU, the residual where the trunk has one); us = median of alternating rounds;')
    say('# +-: max - min of the fp32 arm\'s per-round figures; t1 / t2: bf16x1 tile forms 128x64 / 64x64 (* = the automatic choice);')
    say('# floor: (fp32 activations in + out + residual + bf16 weights) / %.0f TB/s; errors: GEMM without epilogue against fp64' % HBM_TBS)
    # the conv3 shapes carry the block's residual in the trunk, the conv1 shapes (N -> N / 4, on the tap itself) do not
    shapes = [('256->1024 +res', 'layer4', R.layer3[1], True), ('1024->256', 'layer4', R.layer3[2], False),
              ('64->256 +res', 'layer2', R.layer1[1], True), ('128->512 +res', 'layer3', R.layer2[1], True), ('512->2048 +res', 'layer5', R.layer4[1], True),
              ('256->64', 'layer2', R.layer1[2], False), ('512->128', 'layer3', R.layer2[2], False), ('2048->512', 'layer5', R.layer4[2], False)]
    say('%-14s %2s %8s %6s %8s %6s %8s %8s %8s %9s %8s  %-30s %10s %10s %10s %10s' % (
        'shape', 'B', 'map', 'cols', 'fp32 us', '+-', 't1 us', 't2 us', 'floor us', 'fp32/auto', 'MHz f/b', 'fp32 kernel', 'max e f32', 'max e b1',
        'rms e f32', 'rms e b1'))
    verdicts = []
    for name, tap, blk, with_res in shapes:
        t = taps[tap]
        w1, s1, b1 = folded(blk.conv1, blk.bn1)
        if not with_res:
            w, sc, sh = w1, s1, b1
            x8 = t
        else:
            wp1, kt1, _ = ops.pack_weights(w1.to(DEV))
            x8 = ops.conv2d(t, wp1, w1.shape[0], 1, 1, 0, ktab=kt1, scale=s1.to(DEV), shift=b1.to(DEV), relu=True)
            w, sc, sh = folded(blk.conv3, blk.bn3)
        cout, cin = w.shape[0], w.shape[1]
        wd, scd, shd = w.to(DEV), sc.to(DEV), sh.to(DEV)
        wT, kt, lay = ops.pack_weights(wd)
        wB, _, layB = ops.pack_weights(wd, bf16x1=True)
        for B in (8, 1):
            x = x8[:B].contiguous()
            hh, ww = x.shape[2], x.shape[3]
            cols = B * hh * ww
            res = torch.randn(B, cout, hh, ww, generator=g).to(DEV) if with_res else None
            y32 = torch.empty(B, cout, hh, ww, device=DEV)
            yb = torch.empty_like(y32)
            f32 = lambda: ops.conv2d(x, wT, cout, 1, 1, 0, ktab=kt, scale=scd, shift=shd, residual=res, relu=True, out=y32, w_layout=lay)  # noqa: E731

            def fb(tile):
                return lambda: ops.conv2d(x, wB, cout, 1, 1, 0, scale=scd, shift=shd, residual=res, relu=True, out=yb, w_layout=layB, tile=tile)
            f32()
            k32 = H.lib().frtm_conv_last_kernels().decode()
            fb(0)()
            auto = 1 if '<128,' in H.lib().frtm_conv_last_kernels().decode() else 2
            n = max(5, int(2e4 / max(1.0, 2.0 * cout * cin * cols / 1e9)))
            if QUICK:
                n = max(3, n // 4)
            (t32, sp32), (tb1, _), (tb2, _) = ab([f32, fb(1), fb(2)], n, 3 if QUICK else 7)
            mhz32, mhzb = clock_under(f32, n), clock_under(fb(1 if tb1 <= tb2 else 2), n)
            floor = 4.0 * cols * (cin + cout * (2 if with_res else 1)) / (HBM_TBS * 1e12) * 1e6 + 2.0 * cin * cout / (HBM_TBS * 1e12) * 1e6
            X = x.double().reshape(B, cin, -1)
            ref = torch.matmul(wd.double().reshape(cout, cin), X)
            g32 = ops.conv2d(x, wT, cout, 1, 1, 0, ktab=kt, w_layout=lay).double().reshape(B, cout, -1)
            gb = ops.conv2d(x, wB, cout, 1, 1, 0, w_layout=layB).double().reshape(B, cout, -1)
            e32, eb = (g32 - ref).abs(), (gb - ref).abs()
            tauto = tb1 if auto == 1 else tb2
            say('%-14s %2d %8s %6d %8.1f %6.1f %7.1f%s %7.1f%s %8.1f %9.2f %4.0f/%4.0f  %-30s %10.3e %10.3e %10.3e %10.3e' % (
                name, B, '%dx%d' % (hh, ww), cols, t32, sp32, tb1, '*' if auto == 1 else ' ', tb2, '*' if auto == 2 else ' ', floor, t32 / tauto,
                mhz32, mhzb, k32.split()[0], float(e32.max()), float(eb.max()), float(e32.pow(2).mean().sqrt()), float(eb.pow(2).mean().sqrt())))
            verdicts.append('%s B=%d (%d columns): %s (fp32 %.1f +- %.1f, bf16x1 automatic form %.1f)' % (
                name, B, cols, 'FASTER' if t32 - tauto > sp32 else 'not faster', t32, sp32, tauto))
            del X, ref, g32, gb, e32, eb
    say('# routing verdicts (the automatic form is what a trunk launches): faster = fp32 median - bf16x1 median > the fp32 arm\'s spread')
    for v in verdicts:
        say('#   ' + v)
    # whole trunk passes
    say('# ResNet-101 trunk pass (all five taps), eager, median of alternating rounds, routing as compiled (csrc/trunk_route.h: kTrunkRules)')
    img16 = torch.cat([img8, img8.roll(7, dims=3)])
    for B, lanes in ((16, 2), (8, 2), (1, 1)):                 # 16 frames in 2 lanes: the tracker's trunk batches (feature_batch 16)
        ext.lanes = lanes
        img = img16[:B].contiguous()

        def run(mode):
            def f():
                if ext.precision != mode:
                    ext.precision = mode
                ext(img)
            return f
        n = 10 if QUICK else 30
        t = [[], []]
        for _ in range(3 if QUICK else 5):
            for i, mode in enumerate(('fp32', 'bf16x1')):
                run(mode)()
                t[i].append(timed(run(mode), n))
        launches0 = H.lib().frtm_conv_bf16x1_launches()
        ext.precision = 'bf16x1'
        tb = {k: v.clone() for k, v in ext(img).items()}
        torch.cuda.synchronize()
        routed = H.lib().frtm_conv_bf16x1_launches() - launches0
        ext.precision = 'fp32'
        t32 = ext(img)
        rel = ' '.join('%s %.1e' % (k, float((tb[k] - t32[k]).abs().max() / t32[k].abs().max())) for k in sorted(tb))
        a, b = statistics.median(t[0]), statistics.median(t[1])
        say('B=%d lanes=%d: fp32 %.0f us (+- %.0f), bf16x1 %.0f us (%.3fx); %d convs routed per pass; taps max |bf16x1 - fp32| / max |fp32|: %s' % (
            B, lanes, a, max(t[0]) - min(t[0]), b, a / b, routed, rel))
        del tb, t32
    del ext, taps
    torch.cuda.empty_cache()
    trunk_vs_oracle()
    if '--no-tracker' not in sys.argv:
        tracker_fps()
    else:
        say('Tracker frames/s: not measured in this run')
    if '--no-jf' not in sys.argv:
        jf_shift()
    else:
        say('J&F shift: not measured in this run')
    print('wrote', OUT)


def tracker_fps():
    """Frames/s at the headline configuration (ResNet-101, 480x854, 2 objects) per trunk precision, alternating: Tracker.run_sequence (windows,
    batched trunk) and Tracker.track() frame by frame (bench.py: streaming_leg)."""
    import oracle.make_golden_jf as JF
    from oracle.tracker_ref import shift_flip_augment
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    n_frames = 24 if QUICK else 48
    seq = SyntheticSequence('bf16x1', n_frames, (480, 854), 2, seed=7)
    seq.preload(DEV)
    modes = ('fp32', 'bf16x1')
    trk = {}
    for mode in modes:
        params = Parameters(None, device=DEV, feature_extractor='resnet101', trunk_precision=mode)
        refiner = JF.refiner_for('resnet101')
        params.refiner_factory = lambda chans, r=refiner: copy.deepcopy(r)
        params.disc_params.update(**JF.DISC)
        trk[mode] = params.get_model().eval()
        trk[mode].augment = shift_flip_augment
        trk[mode].start_weights = lambda oid: JF.start_weights(7, oid)
        trk[mode].run_sequence(seq)                 # warm-up: graphs captured, workspaces grown
    fps = {m: [] for m in modes}
    routed = 0
    for _ in range(2 if QUICK else 3):
        for mode in modes:
            torch.cuda.synchronize()
            n0 = H.lib().frtm_conv_bf16x1_launches()
            t0 = time.time()
            trk[mode].run_sequence(seq)
            torch.cuda.synchronize()
            fps[mode].append(n_frames / (time.time() - t0))
            if mode == 'bf16x1':
                routed = H.lib().frtm_conv_bf16x1_launches() - n0
    a, b = statistics.median(fps['fp32']), statistics.median(fps['bf16x1'])
    say('Tracker.run_sequence, ResNet-101, 480x854, 2 objects, %d frames (first-frame fit included), median of alternating runs: fp32 %.1f frames/s '
        '(runs %s), bf16x1 %.1f frames/s (%.3fx); %d bf16x1 launches per bf16x1 run (graph replays not counted)' % (
            n_frames, a, ' '.join('%.1f' % v for v in fps['fp32']), b, b / a, routed))
    # frame by frame
    sfps = {m: [] for m in modes}
    own = torch.cuda.Stream(device=DEV)
    frames = [seq[t][0] for t in range(len(seq.images))]
    for rnd in range(3 if QUICK else 4):               # round 0 warms up (graphs of the single-frame pass)
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
    say('Tracker.track() frame by frame (one-frame trunk passes), %d frames: fp32 %.1f frames/s (runs %s), bf16x1 %.1f frames/s (%.3fx)' % (
        len(frames) - 1, a, ' '.join('%.1f' % v for v in sfps['fp32']), b, b / a))
    seq.release()
    del trk
    torch.cuda.empty_cache()


def jf_shift():
    """Dataset-level J&F of the HIP path on the sequences of fixture G14 (tests/test_north_star_gpu.py: _dataset_jf) with an fp32 and a bf16x1 trunk."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_north_star_gpu as NS
    make = NS._hip_tracker
    res = {}
    try:
        for mode in ('fp32', 'bf16x1'):
            def patched(*a, _mode=mode, **kw):
                trk = make(*a, **kw)
                trk.feature_extractor.precision = _mode
                return trk
            NS._hip_tracker = patched
            n0 = H.lib().frtm_conv_bf16x1_launches()
            hip, ora, agree, n_seq = NS._dataset_jf('g14_jf_float32.npz', 'v2', 'jg%02d', (0,))
            res[mode] = (100 * float(hip.mean()), 100 * float(ora.mean()), agree, n_seq, hip.shape[0], H.lib().frtm_conv_bf16x1_launches() - n0)
    finally:
        NS._hip_tracker = make
    f, b = res['fp32'], res['bf16x1']
    say('J&F on the %d sequences (%d objects) of fixture G14, one run each: fp32 HIP path %.3f, bf16x1 HIP path %.3f (shift %+.3f); recorded oracle %.3f; '
        'label agreement with the oracle fp32 %.5f, bf16x1 %.5f; %d bf16x1 launches in the bf16x1 run (graph replays not counted).  '
        'The oracle\'s own single-run sigma: 0.064-0.067 (README)' % (f[3], f[4], f[0], b[0], b[0] - f[0], f[1], f[2], b[2], b[5]))


if __name__ == '__main__':
    main()
