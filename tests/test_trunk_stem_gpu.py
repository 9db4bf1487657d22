"""The trunk's stem and lane slicing on the GPU (csrc/backbone.hip): k_normalize_u8, the 7x7 stem conv, k_maxpool3s2_x4, k_maxpool3s2 and the
per-lane batch slices of frtm_backbone_forward_at, through ResnetFeatureExtractor.

With delta weights, BN folded to scale 1 / shift 0 and the normalisation set to scale 1 / bias 0, layer1 is an integer function of the uint8
frame (tests/_stem_refs.py, which tests/test_trunk_stem.py holds to F.conv2d + F.max_pool2d at float64): tests (a), (b), (c) and (e) compare
with torch.equal, and (f) compares a lane's slice with a plain call on the same frames, bit for bit.  Asking for ['layer1'] stops the pass
after the three stem launches.  The only tolerance in this file is the gate of (d), the stem with real weights against float64:
err <= max(4 x the error of the same three lines in fp32 on the CPU, 1e-6 max|ref|) (tests/test_refiner_train_gpu.py: _gate).

Shapes: SIZES = every (H, W) of 32..43 x 33..48 reaches every branch of the pool's 16-byte / scalar-tail split, both parities of the stem
output and every tail quad of the normaliser; WIDE adds the normaliser's grid-stride loop and a second block in x of either pool
(test_trunk_stem.py: test_sizes_and_wide_reach_every_branch_class)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import _stem_refs as S

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V1_EXTRA = (40, 1031)                             # Wo = 258: five blocks in x of the one-column-per-thread pool


def _report(failed):
    return '%d sizes differ: %s; the first (size, (frame, channel, y, x, got, want)): %s' % (len(failed), sorted(f[0] for f in failed), failed[:4])


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ts', (0, 1, 2))
def test_exact_stem_at_every_edge(ts):
    ext = S.delta_trunk(S.TAP_SETS[ts], DEV)
    failed = S.check_sizes(ext, S.TAP_SETS[ts], S.SIZES)
    assert not failed, _report(failed)


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------------
def test_exact_stem_wide():
    """The normaliser's second trip through its grid-stride loop, the second x block of the pool and blockIdx.z up to 511."""
    B, H, W = S.WIDE
    assert {'grid-stride loop', 'x4 second x block'} <= S.branch_classes(H, W, B)
    ext = S.delta_trunk(S.TAP_SETS[0], DEV)
    img = S.frames(0, H, W, B)
    got = ext(img.to(DEV), ['layer1'])['layer1'].cpu()
    assert got.shape == (B, 64) + S.out_size(H, W)
    for b in range(B):
        want = S.stem_exact(img[b], S.TAP_SETS[0]).to(torch.float32)
        assert torch.equal(got[b:b + 1], want), (b, S.first_difference(got[b:b + 1], want))


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------
def _v1_child():
    """Runs in the child (FRTM_MAXPOOL_V1 is read once per process): the check of (a) for tap set 0 and one wide frame; prints one JSON line."""
    assert os.environ.get('FRTM_MAXPOOL_V1')
    ext = S.delta_trunk(S.TAP_SETS[0], DEV)
    failed = S.check_sizes(ext, S.TAP_SETS[0], S.SIZES)
    failed += S.check_sizes(ext, S.TAP_SETS[0], [V1_EXTRA], B=1)
    print('V1POOL ' + json.dumps({'sizes': len(S.SIZES) + 1, 'failed': failed}))
    return 1 if failed else 0


def test_v1_pool_in_a_child_process():
    """k_maxpool3s2 (FRTM_MAXPOOL_V1) promises the maxima of the x4 kernel: the same exact check.  One fresh child; a child that dies on a
    signal or runs into the time limit fails the test."""
    assert 'v1 second x block' in S.branch_classes(V1_EXTRA[0], V1_EXTRA[1], 1)
    env = dict(os.environ, FRTM_MAXPOOL_V1='1', PYTHONPATH=ROOT)
    p = subprocess.run([sys.executable, '-s', os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith('V1POOL ')]
    assert line, p.stdout[-3000:]
    rep = json.loads(line[-1][len('V1POOL '):])
    assert rep == {'sizes': len(S.SIZES) + 1, 'failed': []}, rep


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------
def test_lane_slices_exact():
    """7 frames on 1, 2, 3, 4 and 8 lanes (7, 4+3, 3+2+2, 2+2+2+1, seven lanes of one) and 2 frames on 4 lanes (L = min(lanes, B)), either lane
    set: every frame's layer1 is exact.  The frames change place from call to call, so a slice that no lane wrote cannot hold the right
    values from the call before."""
    H, W, taps = 37, 45, S.TAP_SETS[1]
    ext = S.delta_trunk(taps, DEV)
    img = torch.stack([S.frame(S.KINDS[b % 3], H, W, 70 + b) for b in range(7)])
    want = S.stem_exact(img, taps).to(torch.float32)
    assert all(not torch.equal(want[a], want[b]) for a in range(7) for b in range(a))
    call = 0
    for lanes in (1, 2, 3, 4, 8):
        ext.lanes = lanes
        for lane_set in (0, 1):
            order = [(b + call) % 7 for b in range(7)]
            call += 1
            got = ext(img[order].to(DEV), ['layer1'], lane_set=lane_set)['layer1'].cpu()
            for b in range(7):
                assert torch.equal(got[b], want[order[b]]), (lanes, lane_set, b, S.first_difference(got[b:b + 1], want[order[b]][None]))
    ext.lanes = 4
    for lane_set in (0, 1):
        order = [5 - lane_set, 2 + lane_set]
        got = ext(img[order].to(DEV), ['layer1'], lane_set=lane_set)['layer1'].cpu()
        assert got.shape[0] == 2 and torch.equal(got, want[order]), (lane_set, S.first_difference(got, want[order]))


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ('resnet18', 'resnet50'))
def test_lane_slices_full_depth(name):
    """5 frames of 37x45 on 3 lanes (2+2+1): every tap's frames 0:2, 2:4 and 4:5 equal a one-lane call on those frames alone, bit for bit
    (the per-lane batch is the same, so the routes are).  At 37x45 every level of the tap pyramid rounds up (19x23, 10x12, 5x6, 3x3, 2x2),
    with 64 << s channels (resnet18) and four times as many (resnet50)."""
    from oracle import cpu_ref as O
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    ext = ResnetFeatureExtractor(name, weights=O.resnet_random_params(name, 2)).to(DEV)
    keep = []                                                          # earlier outputs stay allocated: a new one never lands on their values
    for lane_set in (0, 1):
        img = torch.stack([S.frame(S.KINDS[b % 3], 37, 45, 100 * lane_set + b) for b in range(5)]).to(DEV)
        ext.lanes = 1
        ref = [ext(img[a:b], lane_set=lane_set) for a, b in ((0, 2), (2, 4), (4, 5))]
        ext.lanes = 3
        out = ext(img, lane_set=lane_set)
        keep += [ref, out]
        assert sorted(out) == ['layer1', 'layer2', 'layer3', 'layer4', 'layer5']
        for L in out:
            assert out[L].shape[0] == 5 and bool(torch.isfinite(out[L]).all()), L
            for (a, b), r in zip(((0, 2), (2, 4), (4, 5)), ref):
                assert torch.equal(out[L][a:b], r[L]), (lane_set, L, a, S.first_difference(out[L][a:b].cpu(), r[L].cpu()))
        assert not torch.equal(out['layer5'][0], out['layer5'][2])


# ---- (d), after the exact ones -------------------------------------------------------------------------------------------------------------
def test_stem_real_arithmetic():
    """ImageNet normalisation and seeded weights against the float64 stem, element by element (ReLU and max are continuous: nothing is
    excluded), at the 16 widths of SIZES and H = 33, 38."""
    from oracle import cpu_ref as O
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    P = O.resnet_random_params('resnet18', 5)
    ext = ResnetFeatureExtractor('resnet18', weights=P).to(DEV)
    worst, missed = 0.0, []
    for i, (H, W) in enumerate((H, W) for H in (38, 33) for W in range(48, 32, -1)):
        img = S.frames(i, H, W)
        got = ext(img.to(DEV), ['layer1'])['layer1'].double().cpu()
        ref = S.stem_fp(img, P, torch.float64)['layer1']
        t32 = S.stem_fp(img, P, torch.float32)['layer1'].double()
        err, e32 = float((got - ref).abs().max()), float((t32 - ref).abs().max())
        bound = max(4 * e32, 1e-6 * float(ref.abs().max()))
        print('stem %dx%d: hip err %.3e, torch32 err %.3e, bound %.3e, err / bound %.3f' % (H, W, err, e32, bound, err / bound))
        worst = max(worst, err / bound)
        if not err <= bound:
            missed.append((H, W, err, bound))
    print('stem real arithmetic: worst err / bound %.3f' % worst)
    assert not missed, missed


if __name__ == '__main__':
    sys.path.insert(0, ROOT)
    sys.exit(_v1_child())
