"""The bf16x1_3x3 trunk mode (FRTM_WLAYOUT_BF16X1_3X3 / _S2 for the trunk's 3x3 convs, Parameters(trunk_precision='bf16x1_3x3')) against the fp32 and
the bf16x1 trunk: kernel times of every 3x3 conv shape of ResNet-18 and ResNet-101 at 1 and 8 frames of 480x854 against the fp32 form the trunk takes
for it, their error against fp64, the bytes-over-bandwidth floor of each launch, whole trunk passes of both trunks, tracker frames/s
(Tracker.run_sequence and frame-by-frame track()), the taps against the CPU oracle, the ResNet-18 trunk against the emulation of
tests/test_bf16x1_trunk3x3_gpu.py and the dataset-level J&F on the sequences of fixture G14.  Writes profiles/bf16x1_trunk3x3_time.txt.

Operands are trunk activations of synthetic 480x854 frames (the clock drops on random data): taps of seeded passes, through the conv1 + BN + ReLU of
a bottleneck block for ResNet-101's 3x3 convs; weights are that block's 3x3 conv (BN folded).  The arms alternate in one process.  The routing rule
of csrc/trunk_route.h (kTrunkRules) is read off the per-shape table: a shape is routed only where the bf16 median (automatic tile form) beats the
median of the fp32 form by more than the spread (max - min) of the fp32 arm's own per-round figures in this run.
    python tools/bf16x1_trunk3x3_time.py [--quick] [--sections shapes,passes,oracle,emulation,tracker,jf] [--append]"""
import copy
import ctypes
import os
import statistics
import sys
import time

import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd import _hip as H, ops  # noqa: E402
from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor  # noqa: E402

DEV = 'cuda:0'
QUICK = '--quick' in sys.argv
SECTIONS = sys.argv[sys.argv.index('--sections') + 1].split(',') if '--sections' in sys.argv else ['shapes', 'passes', 'oracle', 'emulation', 'tracker', 'jf']
OUT = os.path.join(ROOT, 'profiles', 'bf16x1_trunk3x3_time.txt')
HBM_TBS = 8.0                 # MI355X peak HBM bandwidth, TB/s: the floor below is bytes / this
MODES = ('fp32', 'bf16x1', 'bf16x1_3x3')
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


FORM_NAMES = {1: 'halo', 2: 'wino', 3: 'wino4', 4: 'wino6'}          # FRTM_WLAYOUT_HALO3X3, _WINO3X3, _WINO4, _WINO6


def trunk_form(ext, cin, cout, stride, B, hi, wi):
    """The fp32 form the trunk `ext` (in fp32 mode) takes for its 3x3 pad-1 conv of this shape on B images of hi x wi, asked from its own handle
    (frtm_backbone_conv_route): 'wino6' / 'wino4' (three launches), 'wino' (fused F(2x2,3x3)) or 'halo' (the direct kernel, the only form of a
    stride-2 conv)."""
    info, out3 = (ctypes.c_int * 6)(), (ctypes.c_int * 3)()
    for idx in range(H.lib().frtm_backbone_num_convs(ext._handle)):
        H.call_nostream('frtm_backbone_conv_info', ext._handle, idx, info)
        if tuple(info[:4]) == (cout, cin, 3, stride):
            H.call_nostream('frtm_backbone_conv_route', ext._handle, idx, B, hi, wi, out3)
            return FORM_NAMES[out3[0]]
    raise ValueError('%s has no 3x3 conv %d -> %d of stride %d' % (ext.name, cin, cout, stride))


def shapes_section():
    g = torch.Generator().manual_seed(0)
    img8 = torch.randint(0, 256, (8, 3, 480, 854), dtype=torch.uint8, generator=g).to(DEV)
    cases = []          # (name, x8, weights, scale, shift, stride, the trunk the conv belongs to)
    for arch in ('resnet101', 'resnet18'):
        ext = ResnetFeatureExtractor(arch, seed=0).to(DEV)
        ext.lanes = 2
        taps = {k: v.clone() for k, v in ext(img8).items()}
        R = ext.resnet
        for s in range(4):
            layer = getattr(R, 'layer%d' % (s + 1))
            own, prev = taps['layer%d' % (s + 2)], taps['layer%d' % (s + 1)]
            if arch == 'resnet101':
                # stride 1: block 1's conv2 on relu(bn1(conv1(tap))); stride 2: block 0's conv2 on relu(bn1(conv1(previous tap))) (v1.5: the stride sits on the 3x3)
                todo = [(layer[1], own, 1)] + ([(layer[0], prev, 2)] if s else [])
                for blk, t, stride in todo:
                    w1, s1, b1 = folded(blk.conv1, blk.bn1)
                    wp1, kt1, _ = ops.pack_weights(w1.to(DEV))
                    x8 = ops.conv2d(t, wp1, w1.shape[0], 1, 1, 0, ktab=kt1, scale=s1.to(DEV), shift=b1.to(DEV), relu=True)
                    w, sc, sh = folded(blk.conv2, blk.bn2)
                    cases.append(('rn101 %d->%d s%d' % (w.shape[1], w.shape[0], stride), x8, w, sc, sh, stride, ext))
            else:
                # the stride-1 shapes are ResNet-101's (N -> N on the stage's map): measured once, above; stride 2: block 0's conv1 on the previous tap
                if s:
                    w, sc, sh = folded(layer[0].conv1, layer[0].bn1)
                    cases.append(('rn18 %d->%d s2' % (w.shape[1], w.shape[0]), prev, w, sc, sh, 2, ext))
    say('%-18s %2s %8s %6s %-6s %8s %6s %8s %8s %8s %9s %9s  %-46s %10s %10s %10s %10s' % (
        'shape', 'B', 'out map', 'cols', 'form', 'fp32 us', '+-', 't64 us', 't96 us', 'floor us', 'fp32/auto', 'MHz f/b', 'fp32 kernels', 'max e f32', 'max e b1',
        'rms e f32', 'rms e b1'))
    verdicts = []
    for name, x8, w, sc, sh, stride, ext in cases:
        cout, cin = w.shape[0], w.shape[1]
        wd, scd, shd = w.to(DEV), sc.to(DEV), sh.to(DEV)
        wB, _, layB = ops.pack_weights(wd, bf16x1=True, stride=stride)
        packs = {}
        for B in (8, 1):
            x = x8[:B].contiguous()
            hi, wi = x.shape[2], x.shape[3]
            ho, wo = (hi - 1) // stride + 1, (wi - 1) // stride + 1
            cols = B * ho * wo
            form = trunk_form(ext, cin, cout, stride, B, hi, wi)
            if form not in packs:
                packs[form] = ops.pack_weights(wd, wino=form == 'wino', wino4=form == 'wino4', wino6=form == 'wino6')
            wT, kt, lay = packs[form]
            ws = ops.wino4_workspace(B, cin, cout, ho, wo, DEV, m=int(form[4])) if form in ('wino4', 'wino6') else None
            y32 = torch.empty(B, cout, ho, wo, device=DEV)
            yb = torch.empty_like(y32)
            sk = 0 if form == 'halo' else 1
            f32 = lambda: ops.conv2d(x, wT, cout, 3, stride, 1, ktab=kt, scale=scd, shift=shd, relu=True, out=y32, w_layout=lay, ws=ws, splitk=sk)  # noqa: E731

            def fb(tile):
                return lambda: ops.conv2d(x, wB, cout, 3, stride, 1, scale=scd, shift=shd, relu=True, out=yb, w_layout=layB, tile=tile)
            f32()
            k32 = H.lib().frtm_conv_last_kernels().decode()
            fb(0)()
            auto = 2 if '<3>' in H.lib().frtm_conv_last_kernels().decode() else 1
            n = max(5, int(2e4 / max(1.0, 2.0 * 9 * cout * cin * cols / 1e9)))
            if QUICK:
                n = max(3, n // 4)
            (t32, sp32), (tb1, _), (tb2, _) = ab([f32, fb(1), fb(2)], n, 3 if QUICK else 7)
            mhz32, mhzb = clock_under(f32, n), clock_under(fb(auto), n)
            floor = (4.0 * B * (cin * hi * wi + cout * ho * wo) + 2.0 * 9 * cin * cout) / (HBM_TBS * 1e12) * 1e6
            # error of the bare conv against fp64, on the first image (fp64 on the CPU)
            ref = F.conv2d(x[:1].double().cpu(), wd.double().cpu(), stride=stride, padding=1)
            g32 = ops.conv2d(x[:1].contiguous(), wT, cout, 3, stride, 1, ktab=kt, w_layout=lay, splitk=sk,
                             ws=ops.wino4_workspace(1, cin, cout, ho, wo, DEV, m=int(form[4])) if form in ('wino4', 'wino6') else None).double().cpu()
            gb = ops.conv2d(x[:1].contiguous(), wB, cout, 3, stride, 1, w_layout=layB).double().cpu()
            e32, eb = (g32 - ref).abs(), (gb - ref).abs()
            tauto = tb1 if auto == 1 else tb2
            say('%-18s %2d %8s %6d %-6s %8.1f %6.1f %7.1f%s %7.1f%s %8.1f %9.2f %4.0f/%4.0f  %-46s %10.3e %10.3e %10.3e %10.3e' % (
                name, B, '%dx%d' % (ho, wo), cols, form, t32, sp32, tb1, '*' if auto == 1 else ' ', tb2, '*' if auto == 2 else ' ', floor, t32 / tauto,
                mhz32, mhzb, k32[:46], float(e32.max()), float(eb.max()), float(e32.pow(2).mean().sqrt()), float(eb.pow(2).mean().sqrt())))
            verdicts.append('%s B=%d (%d columns): %s (fp32 %s %.1f +- %.1f, bf16 automatic form %.1f)' % (
                name, B, cols, 'FASTER' if t32 - tauto > sp32 else 'not faster', form, t32, sp32, tauto))
    say('# routing verdicts (the automatic form is what a trunk launches): faster = fp32 median - bf16 median > the fp32 arm\'s spread')
    for v in verdicts:
        say('#   ' + v)


def passes_section():
    g = torch.Generator().manual_seed(0)
    img8 = torch.randint(0, 256, (8, 3, 480, 854), dtype=torch.uint8, generator=g).to(DEV)
    img16 = torch.cat([img8, img8.roll(7, dims=3)])
    say('# trunk pass (all five taps), eager, median of alternating rounds, routing as compiled (csrc/trunk_route.h: kTrunkRules)')
    for arch in ('resnet101', 'resnet18'):
        ext = ResnetFeatureExtractor(arch, seed=0).to(DEV)
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
            t = {m: [] for m in MODES}
            for _ in range(3 if QUICK else 5):
                for mode in MODES:
                    run(mode)()
                    t[mode].append(timed(run(mode), n))
            routed, taps = {}, {}
            L = H.lib()
            for mode in MODES:
                c0 = (L.frtm_conv_bf16x1_launches(), L.frtm_conv_bf16x1_3x3_launches(), L.frtm_conv_bf16x1_3x3s2_launches())
                ext.precision = mode
                taps[mode] = {k: v.clone() for k, v in ext(img).items()}
                torch.cuda.synchronize()
                routed[mode] = (L.frtm_conv_bf16x1_launches() - c0[0], L.frtm_conv_bf16x1_3x3_launches() - c0[1], L.frtm_conv_bf16x1_3x3s2_launches() - c0[2])
            ext.precision = 'fp32'
            rel = ' '.join('%s %.1e' % (k, float((taps['bf16x1_3x3'][k] - taps['fp32'][k]).abs().max() / taps['fp32'][k].abs().max())) for k in sorted(taps['fp32']))
            med = {m: statistics.median(t[m]) for m in MODES}
            say('%s B=%d lanes=%d: fp32 %.0f us (+- %.0f), bf16x1 %.0f us (%.3fx), bf16x1_3x3 %.0f us (%.3fx of fp32, %.3fx of bf16x1); convs routed per pass '
                '(1x1 / 3x3 s1 / 3x3 s2): bf16x1 %d/%d/%d, bf16x1_3x3 %d/%d/%d; taps max |bf16x1_3x3 - fp32| / max |fp32|: %s' % (
                    arch, B, lanes, med['fp32'], max(t['fp32']) - min(t['fp32']), med['bf16x1'], med['fp32'] / med['bf16x1'], med['bf16x1_3x3'],
                    med['fp32'] / med['bf16x1_3x3'], med['bf16x1'] / med['bf16x1_3x3'], *routed['bf16x1'], *routed['bf16x1_3x3'], rel))
            del taps
        del ext
        torch.cuda.empty_cache()


def oracle_section():
    """Taps against the CPU oracle (oracle/cpu_ref.py) per mode: max |tap - oracle| / max |oracle| per tap.  Recorded, not gated."""
    from oracle import cpu_ref as O
    say('# taps against the CPU oracle (seeded weights, 480x854), max |tap - oracle| / max |oracle|, fp32 / bf16x1 / bf16x1_3x3; one lane, routing as compiled')
    for arch, nb in (('resnet101', 2 if QUICK else 8), ('resnet18', 2 if QUICK else 8)):
        P = O.resnet_random_params(arch, seed=3)
        img = torch.randint(0, 256, (nb, 3, 480, 854), dtype=torch.uint8, generator=torch.Generator().manual_seed(5))
        ref = O.resnet_forward(arch, P, img)
        ext = ResnetFeatureExtractor(arch, weights=P).to(DEV)
        ext.lanes = 1

        def rel(a, b):
            a, b = a.detach().double().cpu(), b.detach().double().cpu()
            return float((a - b).abs().max() / (b.abs().max() + 1e-30))
        for B in (nb, 1):
            out = {}
            for mode in MODES:
                ext.precision = mode
                out[mode] = {k: v.cpu() for k, v in ext(img[:B].to(DEV)).items()}
            say('%s B=%d: %s' % (arch, B, '  '.join('%s %.2e / %.2e / %.2e' % ((k,) + tuple(rel(out[m][k], ref[k][:B]) for m in MODES)) for k in sorted(ref))))
        del ext
        torch.cuda.empty_cache()


def emulation_section():
    """The figures of tests/test_bf16x1_trunk3x3_gpu.py: test_resnet18_trunk_against_the_emulated_roundings, from that test's own code."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_bf16x1_trunk3x3_gpu as T
    torch.set_grad_enabled(False)
    ext = T._with_min_cols(lambda: ResnetFeatureExtractor('resnet18', seed=4).to(DEV))
    ext.lanes = 1
    img = torch.randint(0, 256, (2, 3, 96, 160), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    plain, emu = T._emulate_resnet18(ext, img, False), T._emulate_resnet18(ext, img, True)
    ext.precision = 'bf16x1_3x3'
    hip = {k: v.double().cpu() for k, v in ext(img.to(DEV)).items()}
    say('# ResNet-18 (seed 4, two frames of 96x160, every 3x3 conv routed) against the fp64 emulation of its roundings: max|HIP - plain| / max|emulation - plain| per tap; '
        'the test gates at m = %.3f' % T.EMULATION_MARGIN)
    for k in ('layer2', 'layer3', 'layer4', 'layer5'):
        a, b = float((hip[k] - plain[k]).abs().max()), float((emu[k] - plain[k]).abs().max())
        say('%s: %.4e / %.4e = %.3f' % (k, a, b, a / b))
    del ext


def tracker_section():
    """Frames/s per trunk precision, alternating: Tracker.run_sequence (windows, batched trunk) and Tracker.track() frame by frame, for the headline
    configuration (ResNet-101, 480x854, 2 objects) and the fast one (ResNet-18)."""
    import oracle.make_golden_jf as JF
    from oracle.tracker_ref import shift_flip_augment
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    n_frames = 24 if QUICK else 48
    seq = SyntheticSequence('bf16x1_3x3', n_frames, (480, 854), 2, seed=7)
    seq.preload(DEV)
    for arch, fast, cin in (('resnet101', False, 1024), ('resnet18', True, 256)):
        trk = {}
        for mode in MODES:
            params = Parameters(None, fast=fast, device=DEV, feature_extractor=arch, trunk_precision=mode)
            refiner = JF.refiner_for(arch)
            params.refiner_factory = lambda chans, r=refiner: copy.deepcopy(r)
            if not fast:
                params.disc_params.update(**JF.DISC)
            trk[mode] = params.get_model().eval()
            trk[mode].augment = shift_flip_augment
            trk[mode].start_weights = lambda oid, cin=cin: JF.start_weights(7, oid, cin=cin)
            trk[mode].run_sequence(seq)                 # warm-up: graphs captured, workspaces grown
        fps = {m: [] for m in MODES}
        for _ in range(2 if QUICK else 3):
            for mode in MODES:
                torch.cuda.synchronize()
                t0 = time.time()
                trk[mode].run_sequence(seq)
                torch.cuda.synchronize()
                fps[mode].append(n_frames / (time.time() - t0))
        med = {m: statistics.median(fps[m]) for m in MODES}
        say('Tracker.run_sequence, %s%s, 480x854, 2 objects, %d frames (first-frame fit included), median of alternating runs: fp32 %.1f frames/s (runs %s), '
            'bf16x1 %.1f (%.3fx), bf16x1_3x3 %.1f (%.3fx; runs %s)' % (
                arch, ' fast' if fast else '', n_frames, med['fp32'], ' '.join('%.1f' % v for v in fps['fp32']), med['bf16x1'], med['bf16x1'] / med['fp32'],
                med['bf16x1_3x3'], med['bf16x1_3x3'] / med['fp32'], ' '.join('%.1f' % v for v in fps['bf16x1_3x3'])))
        sfps = {m: [] for m in MODES}
        own = torch.cuda.Stream(device=DEV)
        frames = [seq[t][0] for t in range(len(seq.images))]
        for rnd in range(3 if QUICK else 4):               # round 0 warms up (graphs of the single-frame pass)
            for mode in MODES:
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
        med = {m: statistics.median(sfps[m]) for m in MODES}
        say('Tracker.track() frame by frame (one-frame trunk passes), %s%s, %d frames: fp32 %.1f frames/s (runs %s), bf16x1 %.1f (%.3fx), bf16x1_3x3 %.1f (%.3fx)' % (
            arch, ' fast' if fast else '', len(frames) - 1, med['fp32'], ' '.join('%.1f' % v for v in sfps['fp32']), med['bf16x1'], med['bf16x1'] / med['fp32'],
            med['bf16x1_3x3'], med['bf16x1_3x3'] / med['fp32']))
        del trk
        torch.cuda.empty_cache()
    seq.release()


def jf_section():
    """Dataset-level J&F of the HIP path on the sequences of fixture G14 (tests/test_north_star_gpu.py: _dataset_jf) with an fp32 and a bf16x1_3x3 trunk."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_north_star_gpu as NS
    make = NS._hip_tracker
    L = H.lib()
    res = {}
    try:
        for mode in ('fp32', 'bf16x1_3x3'):
            def patched(*a, _mode=mode, **kw):
                trk = make(*a, **kw)
                trk.feature_extractor.precision = _mode
                return trk
            NS._hip_tracker = patched
            n0 = L.frtm_conv_bf16x1_3x3_launches() + L.frtm_conv_bf16x1_3x3s2_launches()
            hip, ora, agree, n_seq = NS._dataset_jf('g14_jf_float32.npz', 'v2', 'jg%02d', (0,))
            res[mode] = (100 * float(hip.mean()), 100 * float(ora.mean()), agree, n_seq, hip.shape[0],
                         L.frtm_conv_bf16x1_3x3_launches() + L.frtm_conv_bf16x1_3x3s2_launches() - n0)
    finally:
        NS._hip_tracker = make
    f, b = res['fp32'], res['bf16x1_3x3']
    say('J&F on the %d sequences (%d objects) of fixture G14 (ResNet-101), one run each: fp32 HIP path %.3f, bf16x1_3x3 HIP path %.3f (shift %+.3f); recorded oracle %.3f; '
        'label agreement with the oracle fp32 %.5f, bf16x1_3x3 %.5f; %d bf16 3x3 launches in the bf16x1_3x3 run (graph replays not counted).  '
        'The oracle\'s own single-run sigma: 0.064-0.067 (README)' % (f[3], f[4], f[0], b[0], b[0] - f[0], f[1], f[2], b[2], b[5]))


def main():
    torch.set_grad_enabled(False)
    if '--append' in sys.argv and os.path.exists(OUT):
        lines.extend(open(OUT).read().rstrip('\n').split('\n'))
    else:
        say('# bf16x1_3x3 trunk mode (csrc/conv3x3_bf16x1.hip, csrc/conv3x3s2_bf16x1.hip) against the fp32 and bf16x1 trunks on MI355X: %s%s' % (
            time.strftime('%Y-%m-%d'), ' (--quick: fewer rounds)' if QUICK else ''))
        say('# operands: activations of seeded ResNet passes on 8 synthetic 480x854 frames; every arm runs the trunk\'s epilogue (BN scale / shift, ReLU);')
        say('# us = median of alternating rounds; +-: max - min of the fp32 arm\'s per-round figures; form: the fp32 form run_conv takes for the launch;')
        say('# t64 / t96: bf16 tile forms (* = the automatic choice); floor: (fp32 activations in + out + bf16 weights) / %.0f TB/s; errors: bare conv of image 0 against fp64' % HBM_TBS)
    for name in SECTIONS:
        {'shapes': shapes_section, 'passes': passes_section, 'oracle': oracle_section, 'emulation': emulation_section, 'tracker': tracker_section,
         'jf': jf_section}[name]()
        torch.cuda.empty_cache()
    print('wrote', OUT)


if __name__ == '__main__':
    main()
