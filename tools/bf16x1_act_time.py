"""The bf16x1_act trunk mode (bf16 storage of the activations between bf16-routed convs, csrc/conv_bf16act.hip, Parameters(trunk_precision=
'bf16x1_act')) against bf16x1_3x3, the mode it extends: per launch, every routed (Cin, Cout, stride) shape of ResNet-101 and ResNet-18 at 1 and 8
frames of 480x854 -- the parent kernel with fp32 operands against the format-aware form with the formats frtm_backbone_act_plan gives that shape --
next to bytes over bandwidth; whole trunk passes; tracker frames/s (Tracker.run_sequence and frame-by-frame track()); how far the taps move; the
ResNet-18 trunk against the emulation of tests/test_bf16x1_act_gpu.py; the dataset-level J&F on fixture G14.  Writes profiles/bf16x1_act_time.txt.

Device events, the arms alternating in one process, medians, each arm's max - min.  Per-launch operands are synthetic post-ReLU activations
(relu of seeded normals), the same tensor in both formats; weights are seeded; every arm runs the trunk's epilogue (scale / shift, residual where
the conv has one, ReLU).
    python tools/bf16x1_act_time.py [--quick] [--sections shapes,passes,taps,emulation,tracker,jf] [--append] [--out FILE]
    python tools/bf16x1_act_time.py --lib OTHER/libfrtm_hip.so --sections passes      (the bf16x1_3x3 arm alone on another build, e.g. the parent commit's)"""
import copy
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from frtm_vos_amd import _hip as H  # noqa: E402

OTHER_LIB = sys.argv[sys.argv.index('--lib') + 1] if '--lib' in sys.argv else None
if OTHER_LIB:
    H.LIB_PATH = os.path.abspath(OTHER_LIB)          # before the first call loads the library
    _other = ctypes.CDLL(H.LIB_PATH)
    for _name in [k for k in H.SIGNATURES if not hasattr(_other, k)]:      # an older build lacks the newest entry points: not bound, not called
        del H.SIGNATURES[_name]
from frtm_vos_amd import ops  # noqa: E402
from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor  # noqa: E402

DEV = 'cuda:0'
QUICK = '--quick' in sys.argv
SECTIONS = sys.argv[sys.argv.index('--sections') + 1].split(',') if '--sections' in sys.argv else ['shapes', 'passes', 'taps', 'emulation', 'tracker', 'jf']
OUT = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(ROOT, 'profiles', 'bf16x1_act_time.txt')
HBM_TBS = 6.3                 # TB/s: the floor below is bytes / this
MODES = ('bf16x1_3x3',) if OTHER_LIB else ('bf16x1_3x3', 'bf16x1_act')
FRAME = (480, 854)
BLOCKS = {18: (2, 2, 2, 2), 101: (3, 4, 23, 3)}
lines = []


def say(s):
    """Prints a line and keeps the profile on disk up to date (a later stage that fails leaves the earlier ones recorded)."""
    print(s, flush=True)
    lines.append(s)
    with open(OUT, 'w') as f:
        f.write('\n'.join(lines) + '\n')


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


def planned_convs(arch, B):
    """[(shape (Cout, Cin, k, stride, pad), (Hin, Win), layout, (in, res, out) formats, has a residual)] of the convs of a bf16x1_act trunk `arch`
    with a bf16 operand at B frames per lane of 480x854, from a handle without weights (frtm_backbone_conv_route, frtm_backbone_act_plan)."""
    L = H.lib()
    bb = ctypes.c_void_p()
    assert L.frtm_backbone_create(arch, ctypes.byref(bb)) == 0
    try:
        assert L.frtm_backbone_set_bf16_pieces(bb, 1) == 0 and L.frtm_backbone_set_bf16x1_3x3(bb, 1) == 0 and L.frtm_backbone_set_bf16_act(bb, 1) == 0
        n = L.frtm_backbone_num_convs(bb)
        info, out3, plan = (ctypes.c_int * 6)(), (ctypes.c_int * 3)(), (ctypes.c_int * (3 * n))()
        shapes = []
        for i in range(n):
            L.frtm_backbone_conv_info(bb, i, info)
            shapes.append(tuple(info[:6]))
        assert L.frtm_backbone_act_plan(bb, B, FRAME[0], FRAME[1], plan, n) == 0
        half = lambda hw: ((hw[0] + 1) // 2, (hw[1] + 1) // 2)          # noqa: E731
        sizes, i, cur = {0: FRAME}, 1, half(half(FRAME))
        for s, nb in enumerate(BLOCKS[arch]):
            for b in range(nb):
                own = half(cur) if (s > 0 and b == 0) else cur
                nconv, strided = (3, 1) if arch >= 50 else (2, 0)
                for j in range(nconv):
                    sizes[i] = cur if j <= strided else own
                    i += 1
                if b == 0 and (s > 0 or arch >= 50):
                    sizes[i] = cur
                    i += 1
                cur = own
        out = []
        for i in range(n):
            f = tuple(plan[3 * i:3 * i + 3])
            if any(f):
                L.frtm_backbone_conv_route(bb, i, B, sizes[i][0], sizes[i][1], out3)
                out.append((shapes[i][:5], sizes[i], out3[0], f, bool(shapes[i][5])))
        return out, sum(1 for i in range(n) if any(plan[3 * i:3 * i + 3])), n
    finally:
        L.frtm_backbone_destroy(bb)


def shapes_section():
    say('%-22s %2s %8s %7s %-9s %9s %6s %9s %6s %8s %8s %8s  %s' % ('shape', 'B', 'in map', 'cols', 'in/res/out', 'fp32 us', '+-', 'plan us', '+-', 'fp32/plan',
                                                                  'floor32', 'floorPl', 'convs of the trunk with these formats'))
    verdicts = []
    for arch in (101, 18):
        for B in (8, 1):
            convs, n_aware, n_all = planned_convs(arch, B)
            say('# ResNet-%d, %d frame(s) per lane: %d of %d convs have a bf16 operand' % (arch, B, n_aware, n_all))
            groups = {}
            for shape, hw, lay, fmt, has_res in convs:
                groups.setdefault((shape, hw, lay, fmt, has_res), 0)
                groups[(shape, hw, lay, fmt, has_res)] += 1
            for ((cout, cin, k, stride, pad), (hi, wi), lay, fmt, has_res), count in sorted(groups.items(), key=lambda kv: (kv[0][1], kv[0][0])):
                g = torch.Generator().manual_seed(cin * 7 + cout)
                ho, wo = (hi + 2 * pad - k) // stride + 1, (wi + 2 * pad - k) // stride + 1
                x = torch.relu(torch.randn(B, cin, hi, wi, generator=g)).to(DEV)
                w = (torch.randn(cout, cin, k, k, generator=g) / (k * k * cin) ** 0.5).to(DEV)
                sc, sh = (torch.rand(cout, generator=g) + 0.5).to(DEV), (torch.randn(cout, generator=g) * 0.1).to(DEV)
                r = torch.relu(torch.randn(B, cout, ho, wo, generator=g)).to(DEV) if has_res else None
                wT = ops.pack_weights(w, bf16x1=True, stride=stride)[0]
                xb, rb = ops.act_to_bf16(x) if fmt[0] else x, (ops.act_to_bf16(r) if fmt[1] else r) if has_res else None
                y32 = torch.empty(B, cout, ho, wo, device=DEV)
                yp = torch.empty(B * cout * ho * wo, device=DEV, dtype=torch.bfloat16) if fmt[2] else torch.empty_like(y32)
                f32 = lambda: ops.conv2d(x, wT, cout, k, stride, pad, scale=sc, shift=sh, residual=r, relu=True, out=y32, w_layout=lay)  # noqa: E731
                fpl = lambda: ops.conv2d(xb, wT, cout, k, stride, pad, scale=sc, shift=sh, residual=rb, relu=True, out=yp, shape=(B, cin, hi, wi), w_layout=lay,  # noqa: E731
                                         in_fmt=fmt[0], res_fmt=fmt[1] if has_res else 0, out_fmt=fmt[2])
                cols = B * ho * wo
                n = max(5, int(2e4 / max(1.0, 2.0 * k * k * cout * cin * cols / 1e9)))
                if QUICK:
                    n = max(3, n // 4)
                (t32, s32), (tpl, spl) = ab([f32, fpl], n, 3 if QUICK else 7)
                wbytes = 2.0 * k * k * cin * cout
                nin, nout = B * cin * hi * wi, B * cout * ho * wo
                fl32 = (4.0 * (nin + nout * (2 if has_res else 1)) + wbytes) / (HBM_TBS * 1e12) * 1e6
                flpl = ((2 if fmt[0] else 4) * nin + ((2 if fmt[1] else 4) * nout if has_res else 0) + (2 if fmt[2] else 4) * nout + wbytes) / (HBM_TBS * 1e12) * 1e6
                name = 'rn%d %d->%d k%d s%d%s' % (arch, cin, cout, k, stride, ' +res' if has_res else '')
                say('%-22s %2d %8s %7d %-9s %9.1f %6.1f %9.1f %6.1f %8.2f %8.1f %8.1f  %d' % (
                    name, B, '%dx%d' % (hi, wi), cols, '%d/%d/%d' % fmt, t32, s32, tpl, spl, t32 / tpl, fl32, flpl, count))
                verdicts.append('%s B=%d formats %d/%d/%d: %s (fp32 operands %.1f +- %.1f, planned formats %.1f +- %.1f)' % (
                    name, B, fmt[0], fmt[1], fmt[2], 'FASTER' if t32 - tpl > max(s32, spl) else 'SLOWER' if tpl - t32 > max(s32, spl) else 'within the spread',
                    t32, s32, tpl, spl))
                del x, w, r, xb, rb, y32, yp
            torch.cuda.empty_cache()
    say('# per-launch verdicts: faster / slower = the medians differ by more than the larger of the two arms\' spreads')
    for v in verdicts:
        say('#   ' + v)


def passes_section():
    g = torch.Generator().manual_seed(0)
    img8 = torch.randint(0, 256, (8, 3) + FRAME, dtype=torch.uint8, generator=g).to(DEV)
    img16 = torch.cat([img8, img8.roll(7, dims=3)])
    say('# trunk pass (all five taps), eager, median of alternating rounds, routing as compiled (csrc/trunk_route.h: kTrunkRules)%s' % (
        '; library: %s -- the bf16x1_3x3 arm alone' % OTHER_LIB if OTHER_LIB else ''))
    for arch in ('resnet101', 'resnet18'):
        ext = ResnetFeatureExtractor(arch, seed=0).to(DEV)
        for B, lanes in ((16, 2), (8, 2), (1, 1)):                 # 16 frames in 2 lanes: the tracker's trunk batches
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
            for _ in range(3 if QUICK else 7):
                for mode in MODES:
                    run(mode)()
                    t[mode].append(timed(run(mode), n))
            med = {m: statistics.median(t[m]) for m in MODES}
            spread = {m: max(t[m]) - min(t[m]) for m in MODES}
            if OTHER_LIB:
                say('%s B=%d lanes=%d: bf16x1_3x3 %.0f us (+- %.0f)' % (arch, B, lanes, med['bf16x1_3x3'], spread['bf16x1_3x3']))
                continue
            c0 = H.lib().frtm_conv_bf16act_launches()
            run('bf16x1_act')()
            torch.cuda.synchronize()
            aware = H.lib().frtm_conv_bf16act_launches() - c0
            d = med['bf16x1_3x3'] - med['bf16x1_act']
            s = max(spread.values())
            say('%s B=%d lanes=%d: bf16x1_3x3 %.0f us (+- %.0f), bf16x1_act %.0f us (+- %.0f): %.3fx, %s; %d format-aware launches per pass of %d' % (
                arch, B, lanes, med['bf16x1_3x3'], spread['bf16x1_3x3'], med['bf16x1_act'], spread['bf16x1_act'], med['bf16x1_3x3'] / med['bf16x1_act'],
                'FASTER by more than the spread' if d > s else 'SLOWER by more than the spread' if -d > s else 'within the spread', aware, ext.last_conv_launches))
        ext.precision = 'fp32'
        del ext
        torch.cuda.empty_cache()


def taps_section():
    """How far each tap moves, relative to its range (max |fp32 tap|): bf16x1_act against the fp32 trunk and against bf16x1_3x3, next to bf16x1_3x3 against fp32."""
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (8, 3) + FRAME, dtype=torch.uint8, generator=g).to(DEV)
    say('# taps of 8 synthetic 480x854 frames in one lane (seeded weights), max |a - b| / max |fp32 tap|: bf16x1_3x3 - fp32 / bf16x1_act - fp32 / bf16x1_act - bf16x1_3x3')
    for arch in ('resnet101', 'resnet18'):
        ext = ResnetFeatureExtractor(arch, seed=0).to(DEV)
        ext.lanes = 1
        taps = {}
        for mode in ('fp32', 'bf16x1_3x3', 'bf16x1_act'):
            ext.precision = mode
            taps[mode] = {k: v.clone() for k, v in ext(img).items()}
        rel = lambda a, b, k: float((taps[a][k] - taps[b][k]).abs().max() / taps['fp32'][k].abs().max())  # noqa: E731
        say('%s: %s' % (arch, '  '.join('%s %.2e / %.2e / %.2e' % (k, rel('bf16x1_3x3', 'fp32', k), rel('bf16x1_act', 'fp32', k), rel('bf16x1_act', 'bf16x1_3x3', k))
                                        for k in sorted(taps['fp32']))))
        del ext, taps
        torch.cuda.empty_cache()


def emulation_section():
    """The figures of tests/test_bf16x1_act_gpu.py: test_resnet18_trunk_against_the_emulated_roundings, from that test's own code."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_bf16x1_act_gpu as T
    ext = T._with_min_cols(lambda: ResnetFeatureExtractor('resnet18', seed=4).to(DEV))
    ext.lanes = 1
    B, Hh, Ww = 2, 96, 160
    img = torch.randint(0, 256, (B, 3, Hh, Ww), dtype=torch.uint8, generator=torch.Generator().manual_seed(9))
    h = T.Trunk(18, bb=ext._handle)
    ext.precision = 'bf16x1_act'
    hip = {k: v.double().cpu() for k, v in ext(img.to(DEV)).items()}
    rounded = {i for i, f in enumerate(h.plan(B, Hh, Ww)) if f[2]}
    plain, emu = T._emulate(ext, h, img, B, Hh, Ww, False, set()), T._emulate(ext, h, img, B, Hh, Ww, True, rounded)
    say('# ResNet-18 (seed 4, two frames of 96x160, every 3x3 conv routed, %d tensors stored as bf16) against the fp64 emulation of its roundings: '
        'max|HIP - plain| / max|emulation - plain| per tap; the test gates at m = %.3f' % (len(rounded), T.EMULATION_MARGIN))
    for k in ('layer2', 'layer3', 'layer4', 'layer5'):
        a, b = float((hip[k] - plain[k]).abs().max()), float((emu[k] - plain[k]).abs().max())
        say('%s: %.4e / %.4e = %.4f' % (k, a, b, a / b))
    del ext


def tracker_section():
    """Frames/s per trunk precision, alternating: Tracker.run_sequence (windows, batched trunk) and Tracker.track() frame by frame, for the headline
    configuration (ResNet-101, 480x854, 2 objects) and the fast one (ResNet-18)."""
    import oracle.make_golden_jf as JF
    from oracle.tracker_ref import shift_flip_augment
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    n_frames = 24 if QUICK else 48
    seq = SyntheticSequence('bf16x1_act', n_frames, FRAME, 2, seed=7)
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
        say('Tracker.run_sequence, %s%s, 480x854, 2 objects, %d frames (first-frame fit included), alternating runs: %s' % (
            arch, ' fast' if fast else '', n_frames, ', '.join('%s median %.1f frames/s (runs %s)' % (m, statistics.median(fps[m]), ' '.join('%.1f' % v for v in fps[m])) for m in MODES)))
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
        say('Tracker.track() frame by frame (one-frame trunk passes), %s%s, %d frames: %s' % (
            arch, ' fast' if fast else '', len(frames) - 1,
            ', '.join('%s median %.1f frames/s (runs %s)' % (m, statistics.median(sfps[m]), ' '.join('%.1f' % v for v in sfps[m])) for m in MODES)))
        del trk
        torch.cuda.empty_cache()
    seq.release()


def jf_section():
    """Dataset-level J&F of the HIP path on the sequences of fixture G14 (tests/test_north_star_gpu.py: _dataset_jf), one run per mode."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import test_north_star_gpu as NS
    make = NS._hip_tracker
    L = H.lib()
    res = {}
    try:
        for mode in ('bf16x1_3x3', 'bf16x1_act'):
            def patched(*a, _mode=mode, **kw):
                trk = make(*a, **kw)
                trk.feature_extractor.precision = _mode
                return trk
            NS._hip_tracker = patched
            n0 = L.frtm_conv_bf16act_launches()
            hip, ora, agree, n_seq = NS._dataset_jf('g14_jf_float32.npz', 'v2', 'jg%02d', (0,))
            res[mode] = (100 * float(hip.mean()), 100 * float(ora.mean()), agree, n_seq, hip.shape[0], L.frtm_conv_bf16act_launches() - n0)
    finally:
        NS._hip_tracker = make
    a, b = res['bf16x1_3x3'], res['bf16x1_act']
    say('J&F on the %d sequences (%d objects) of fixture G14 (ResNet-101), one run each: bf16x1_3x3 HIP path %.3f, bf16x1_act HIP path %.3f (shift %+.3f); recorded oracle %.3f; '
        'label agreement with the oracle bf16x1_3x3 %.5f, bf16x1_act %.5f; %d format-aware launches in the bf16x1_act run (graph replays not counted).  '
        'The oracle\'s own single-run sigma: 0.064-0.067 (README)' % (a[3], a[4], a[0], b[0], b[0] - a[0], a[1], a[2], b[2], b[5]))


def main():
    torch.set_grad_enabled(False)
    if '--append' in sys.argv and os.path.exists(OUT):
        lines.extend(open(OUT).read().rstrip('\n').split('\n'))
    else:
        say('# bf16x1_act trunk mode (csrc/conv_bf16act.hip, csrc/trunk_route.h: act_plan) against bf16x1_3x3 on MI355X: %s%s' % (
            time.strftime('%Y-%m-%d'), ' (--quick: fewer rounds)' if QUICK else ''))
        say('# us = median of alternating rounds; +-: max - min of that arm\'s per-round figures; in/res/out: FRTM_ACT_* of the planned arm (1 = bf16 storage);')
        say('# fp32 us: the parent kernel (conv_bf16x1 / conv3x3_bf16x1 / conv3x3s2_bf16x1) on fp32 operands; plan us: the format-aware form with the planned formats;')
        say('# floor32 / floorPl: bytes of (input + residual + output in their formats + bf16 weights) / %.1f TB/s, us' % HBM_TBS)
    for name in SECTIONS:
        {'shapes': shapes_section, 'passes': passes_section, 'taps': taps_section, 'emulation': emulation_section, 'tracker': tracker_section,
         'jf': jf_section}[name]()
        torch.cuda.empty_cache()
    print('wrote', OUT)


if __name__ == '__main__':
    main()
