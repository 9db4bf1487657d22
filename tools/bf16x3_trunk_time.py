"""The bf16x3 trunk mode (FRTM_WLAYOUT_BF16X3, Parameters(trunk_precision='bf16x3')) against the fp32 trunk: kernel times of the stride-1 1x1 conv
shapes, their error against fp64, whole ResNet-101 trunk passes and tracker frames/s.  Writes profiles/bf16x3_trunk_time.txt.

Operands are trunk activations of synthetic 480x854 frames (the clock drops on random data): the taps of a seeded ResNet-101 pass, through the
conv1 + BN + ReLU of the next block of that stage for the narrow inputs; weights are that block's conv3 (BN folded).  The two arms alternate in
one process; frtm_clock_probe reports the shader clock under each arm's load.
    python tools/bf16x3_trunk_time.py [--quick]"""
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
OUT = os.path.join(ROOT, 'profiles', 'bf16x3_trunk_time.txt')
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


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
    """Alternating rounds of the arms; median us per call of each."""
    t = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            t[i].append(timed(fn, n))
    return [statistics.median(v) for v in t]


def main():
    torch.set_grad_enabled(False)
    g = torch.Generator().manual_seed(0)
    ext = ResnetFeatureExtractor('resnet101', seed=0).to(DEV)
    ext.lanes = 2
    R = ext.resnet
    img8 = torch.randint(0, 256, (8, 3, 480, 854), dtype=torch.uint8, generator=g).to(DEV)
    taps = ext(img8)
    say('# bf16x3 trunk mode (csrc/conv_bf16x3.hip) against the fp32 trunk on MI355X: %s' % time.strftime('%Y-%m-%d'))
    say('# operands: taps of a seeded ResNet-101 pass on 8 synthetic 480x854 frames; narrow inputs = relu(bn(conv1 of block 1)) of the tap')
    # (name, stage tap, block whose conv1 makes the input / whose conv3 is the weight, residual)
    # the conv3 shapes carry the block's residual in the trunk, conv1 (1024 -> 256) does not; every arm runs the trunk's BN + ReLU epilogue
    shapes = [('256->1024 +res', 'layer4', R.layer3[1], True), ('1024->256', 'layer4', R.layer3[2], False),
              ('64->256 +res', 'layer2', R.layer1[1], True), ('128->512 +res', 'layer3', R.layer2[1], True), ('512->2048 +res', 'layer5', R.layer4[1], True)]
    say('%-14s %2s %10s %9s %9s %7s %7s  %-24s %11s %11s %11s %11s' % ('shape', 'B', 'map', 'fp32 us', 'bf16x3 us', 'speedup', 'MHz f/b', 'fp32 kernel',
                                                                       'max err f32', 'max err b3', 'rms err f32', 'rms err b3'))
    ratios = []                          # (max error ratio, rms error ratio) bf16x3 / fp32 of every row
    for name, tap, blk, with_res in shapes:
        t = taps[tap]
        w1, s1, b1 = folded(blk.conv1, blk.bn1)
        if name.startswith('1024->256'):
            w, sc, sh = w1, s1, b1
            x8 = t
        else:
            wp1, kt1, _ = ops.pack_weights(w1.to(DEV))
            x8 = ops.conv2d(t, wp1, w1.shape[0], 1, 1, 0, ktab=kt1, scale=s1.to(DEV), shift=b1.to(DEV), relu=True)
            w, sc, sh = folded(blk.conv3, blk.bn3)
        cout, cin = w.shape[0], w.shape[1]
        wd, scd, shd = w.to(DEV), sc.to(DEV), sh.to(DEV)
        wT, kt, lay = ops.pack_weights(wd)
        wB, _, layB = ops.pack_weights(wd, bf16x3=True)
        for B in (8, 1):
            x = x8[:B].contiguous()
            hh, ww = x.shape[2], x.shape[3]
            res = torch.randn(B, cout, hh, ww, generator=g).to(DEV) if with_res else None
            y32 = torch.empty(B, cout, hh, ww, device=DEV)
            yb = torch.empty_like(y32)
            f32 = lambda: ops.conv2d(x, wT, cout, 1, 1, 0, ktab=kt, scale=scd, shift=shd, residual=res, relu=True, out=y32, w_layout=lay)  # noqa: E731
            fb = lambda: ops.conv2d(x, wB, cout, 1, 1, 0, scale=scd, shift=shd, residual=res, relu=True, out=yb, w_layout=layB)  # noqa: E731
            f32()
            k32 = H.lib().frtm_conv_last_kernels().decode()
            fb()
            n = max(5, int(2e4 / max(1.0, 2.0 * cout * cin * B * hh * ww / 1e9)))
            if QUICK:
                n = max(3, n // 4)
            t32, tb = ab([f32, fb], n, 3 if QUICK else 5)
            mhz32, mhzb = clock_under(f32, n), clock_under(fb, n)
            # error of the GEMM itself (no epilogue) against fp64, on the same data
            X = x.double().reshape(B, cin, -1)
            ref = torch.matmul(wd.double().reshape(cout, cin), X)
            g32 = ops.conv2d(x, wT, cout, 1, 1, 0, ktab=kt, w_layout=lay).double().reshape(B, cout, -1)
            gb = ops.conv2d(x, wB, cout, 1, 1, 0, w_layout=layB).double().reshape(B, cout, -1)
            e32, eb = (g32 - ref).abs(), (gb - ref).abs()
            ratios.append((float(eb.max() / e32.max()), float(eb.pow(2).mean().sqrt() / e32.pow(2).mean().sqrt())))
            say('%-14s %2d %10s %9.1f %9.1f %7.2f %4.0f/%4.0f  %-24s %11.3e %11.3e %11.3e %11.3e' % (
                name, B, '%dx%d' % (hh, ww), t32, tb, t32 / tb, mhz32, mhzb, k32.split()[0], float(e32.max()), float(eb.max()),
                float(e32.pow(2).mean().sqrt()), float(eb.pow(2).mean().sqrt())))
            del X, ref, g32, gb, e32, eb
    say('# error against fp64 of the GEMM (no epilogue), bf16x3 / fp32 over the rows above: max %.2f-%.2fx, rms %.2f-%.2fx' % (
        min(r[0] for r in ratios), max(r[0] for r in ratios), min(r[1] for r in ratios), max(r[1] for r in ratios)))
    # whole trunk passes
    say('# ResNet-101 trunk pass (all five taps), eager, median of alternating rounds')
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
            for i, mode in enumerate(('fp32', 'bf16x3')):
                run(mode)()
                t[i].append(timed(run(mode), n))
        launches0 = H.lib().frtm_conv_bf16x3_launches()
        ext.precision = 'bf16x3'
        ext(img)
        torch.cuda.synchronize()
        routed = H.lib().frtm_conv_bf16x3_launches() - launches0
        a, b = statistics.median(t[0]), statistics.median(t[1])
        say('B=%d lanes=%d: fp32 %.0f us, bf16x3 %.0f us (%.3fx); %d convs routed per pass' % (B, lanes, a, b, a / b, routed))
        ext.precision = 'fp32'
    del ext, taps
    torch.cuda.empty_cache()
    if '--no-tracker' not in sys.argv:
        tracker_fps()
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('wrote', OUT)


def tracker_fps():
    """Frames/s of Tracker.run_sequence at the headline configuration (ResNet-101, 480x854, 2 objects) per trunk precision, alternating."""
    import oracle.make_golden_jf as JF
    from oracle.tracker_ref import shift_flip_augment
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    n_frames = 24 if QUICK else 48
    seq = SyntheticSequence('bf16x3', n_frames, (480, 854), 2, seed=7)
    seq.preload(DEV)
    trk = {}
    for mode in ('fp32', 'bf16x3'):
        params = Parameters(None, device=DEV, feature_extractor='resnet101', trunk_precision=mode)
        refiner = JF.refiner_for('resnet101')
        params.refiner_factory = lambda chans, r=refiner: copy.deepcopy(r)
        params.disc_params.update(**JF.DISC)
        trk[mode] = params.get_model().eval()
        trk[mode].augment = shift_flip_augment
        trk[mode].start_weights = lambda oid: JF.start_weights(7, oid)
        trk[mode].run_sequence(seq)                 # warm-up: graphs captured, workspaces grown
    fps = {'fp32': [], 'bf16x3': []}
    routed = 0
    for _ in range(2 if QUICK else 3):
        for mode in ('fp32', 'bf16x3'):
            torch.cuda.synchronize()
            n0 = H.lib().frtm_conv_bf16x3_launches()
            t0 = time.time()
            trk[mode].run_sequence(seq)
            torch.cuda.synchronize()
            fps[mode].append(n_frames / (time.time() - t0))
            if mode == 'bf16x3':
                routed = H.lib().frtm_conv_bf16x3_launches() - n0
    a, b = statistics.median(fps['fp32']), statistics.median(fps['bf16x3'])
    say('Tracker.run_sequence, ResNet-101, 480x854, 2 objects, %d frames (first-frame fit included), median of alternating runs: fp32 %.1f frames/s, '
        'bf16x3 %.1f frames/s (%.3fx); %d bf16x3 launches per bf16x3 run' % (n_frames, a, b, b / a, routed))
    seq.release()


if __name__ == '__main__':
    main()
