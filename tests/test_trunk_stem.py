"""CPU side of the stem checks of csrc/backbone.hip (k_normalize_u8, the stem conv, k_maxpool3s2_x4 / k_maxpool3s2, the lane slicing).

(a) The integer statement of tests/_stem_refs.py (stem_exact) equals F.max_pool2d(F.relu(F.conv2d(img, w_delta, stride=2, padding=3)), 3, 2, 1)
    at float64 EXACTLY, and stem_fp equals the first tap of oracle/cpu_ref.py: resnet_forward bit for bit.  The GPU tests
    (tests/test_trunk_stem_gpu.py) hold the kernels to these two.
(b) SIZES and WIDE together reach every branch class of the three kernels (branch_classes restates the conditions); the three classes that
    only WIDE reaches are absent from SIZES, so dropping WIDE fails here.
(c) COVERED names, for every __global__ of csrc/backbone.hip, the GPU tests that launch it, or says that it is a timing helper with no
    result to check.  A kernel added without an entry fails test_every_kernel_is_covered.

No tolerance appears in this file."""
import ast
import os
import re

import torch
import torch.nn.functional as F

import _stem_refs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'frtm-vos_amd', 'csrc')
STEM = 'tests/test_trunk_stem_gpu.py::'
B3X3 = 'tests/test_bf16x1_trunk3x3_gpu.py::'

COVERED = {
    'k_normalize_u8': [STEM + 'test_exact_stem_at_every_edge', STEM + 'test_exact_stem_wide', STEM + 'test_stem_real_arithmetic'],
    'k_maxpool3s2_x4': [STEM + 'test_exact_stem_at_every_edge', STEM + 'test_exact_stem_wide', STEM + 'test_stem_real_arithmetic'],
    'k_maxpool3s2': [STEM + 'test_v1_pool_in_a_child_process'],
    # launched when a precision mode turns on after the upload (pack_missing): the 3x3 bf16 images are packed from the halo image
    'k_halo_to_oihw': [B3X3 + 'test_resnet18_trunk_against_the_emulated_roundings', B3X3 + 'test_trunk_routing_counts_round_trip_lanes_and_plan'],
}
# no result to hold to a reference: they keep a queue slot busy / read two clocks for a given time
TIMING_HELPERS = {
    'k_spin': 'frtm-vos_amd/model/tracker.py',           # _streams_are_independent
    'k_clock_probe': 'bench.py',                         # roofline.dominant_kernel
}

GLOBAL_DECL = r'__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?void\s+(\w+)\s*\('
DOZEN = S.SIZES[::17]                                    # (32, 33), (33, 34), .. (43, 44): every parity of h1, w1 and every tail


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the references
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tap_sets_hold_all_147_taps_and_every_plane():
    assert len(S.TAPS) == 147 == len(set(S.TAPS))
    assert len(S.TAP_SETS) == 3
    for c, taps in enumerate(S.TAP_SETS):
        assert len(taps) == 64
        assert taps[:49] == [(c, ky, kx) for ky in range(7) for kx in range(7)]
        assert {t[0] for t in taps} == {0, 1, 2}
        assert set(taps[49:]) == {(o, ky, kx) for o in range(3) if o != c for ky, kx in ((0, 0), (0, 6), (6, 0), (6, 6), (3, 3))}
    assert {t for taps in S.TAP_SETS for t in taps} == set(S.TAPS)


def test_frames_are_what_they_say():
    assert len(DOZEN) == 12
    for kind, ring, lo, hi in (('bright', 255, 0, 127), ('dark', 1, 128, 255)):
        img = S.frame(kind, 33, 41, 5)
        inner = img[:, 4:-4, 4:-4]
        assert img.dtype == torch.uint8 and int(inner.min()) >= lo and int(inner.max()) <= hi
        outer = img.clone()
        outer[:, 4:-4, 4:-4] = ring
        assert bool((outer == ring).all())
    a, b = S.frames(0, 32, 33), S.frames(1, 32, 33)
    assert a.shape == (2, 3, 32, 33) and not torch.equal(a[0], a[1]) and not torch.equal(a, b)
    assert torch.equal(S.frames(7, 35, 40), S.frames(7, 35, 40))      # seeded


def test_stem_exact_is_conv_relu_maxpool_at_float64():
    for i, (H, W) in enumerate(DOZEN):
        img = torch.stack([S.frame(kind, H, W, 10 * i + k) for k, kind in enumerate(S.KINDS)])
        for taps in S.TAP_SETS:
            want = F.max_pool2d(F.relu(F.conv2d(img.double(), S.delta_weights(taps, torch.float64), stride=2, padding=3)), 3, 2, 1)
            got = S.stem_exact(img, taps)
            assert got.dtype == torch.int64 and got.shape == (3, 64) + S.out_size(H, W)
            assert torch.equal(got.double(), want), (H, W, S.first_difference(got.double(), want))
    assert torch.equal(S.stem_exact(img[0], taps), got[:1])           # a single frame


def test_stem_fp_is_the_oracles_first_tap():
    from oracle import cpu_ref as O
    P = O.resnet_random_params('resnet18', 3)
    P64 = {k: v.double() for k, v in P.items()}
    for H, W in ((33, 47), (38, 40)):
        img = S.frames(2, H, W, 3)
        assert torch.equal(S.stem_fp(img, P, torch.float64)['layer1'], O.resnet_forward('resnet18', P64, img, ['layer1'], dtype=torch.float64)['layer1'])
        assert torch.equal(S.stem_fp(img, P, torch.float32)['layer1'], O.resnet_forward('resnet18', P, img, ['layer1'])['layer1'])


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) the shapes reach every branch
# ---------------------------------------------------------------------------------------------------------------------------------
EVERY_CLASS = {
    'full',
    'tail r=1 with right', 'tail r=1 without right', 'tail r=2 with right', 'tail r=2 without right',
    'tail r=3 with right', 'tail r=3 without right', 'tail r=4 without right',
    'w1 odd', 'w1 even', 'h1 odd', 'h1 even',
    'Ho%4=0', 'Ho%4=1', 'Ho%4=2', 'Ho%4=3',
    '(W+6)%4=0', '(W+6)%4=1', '(W+6)%4=2', '(W+6)%4=3',
    'x4 second x block', 'v1 second x block', 'grid-stride loop',
}


def test_sizes_and_wide_reach_every_branch_class():
    assert set(S.ALL_CLASSES) == EVERY_CLASS and len(S.ALL_CLASSES) == len(EVERY_CLASS)
    assert len(S.SIZES) == 192 == len(set(S.SIZES)) and min(min(s) for s in S.SIZES) == 32
    small = set().union(*(S.branch_classes(H, W, 2) for H, W in S.SIZES))
    wide = S.branch_classes(S.WIDE[1], S.WIDE[2], S.WIDE[0])
    only_wide = {'x4 second x block', 'v1 second x block', 'grid-stride loop'}
    assert small == EVERY_CLASS - only_wide
    assert only_wide <= wide and not only_wide & small
    assert small | wide == EVERY_CLASS
    assert 'tail r=2 with right' in wide                               # the second x4 block's only thread


def test_wide_is_just_over_the_normalisers_grid():
    B, H, W = S.WIDE
    quads = B * 3 * (H + 6) * ((W + 6 + 3) // 4)
    assert quads == 2121600 and 8192 * 256 == 2097152
    assert S.out_size(H, W) == (84, 258)
    assert (258 + 63) // 64 == 5 and (258 + 255) // 256 == 2
    assert 'grid-stride loop' not in S.branch_classes(H, W, B - 1)    # one frame fewer stays inside the grid


def test_branch_classes_at_hand_worked_shapes():
    # W = 45: w1 = 23, Wo = 12; thread 2 owns outputs 8..11, x0 = 16, x0 + 7 = 23 is outside: four scalar outputs, the last without a right neighbour
    assert {'full', 'tail r=4 without right', 'w1 odd'} <= S.branch_classes(37, 45, 1)
    # W = 48: w1 = 24, Wo = 12: every thread full, no tail at all
    assert not [c for c in S.branch_classes(37, 48, 1) if c.startswith('tail')]
    # W = 36: w1 = 18, Wo = 9: thread 2 owns output 8 alone, centre column 16, column 17 inside
    assert 'tail r=1 with right' in S.branch_classes(37, 36, 1)
    # H = 37: h1 = 19 odd, Ho = 10
    assert {'h1 odd', 'Ho%4=2', '(W+6)%4=2'} <= S.branch_classes(37, 36, 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the ledger
# ---------------------------------------------------------------------------------------------------------------------------------
def _kernels(name):
    return set(re.findall(GLOBAL_DECL, open(os.path.join(CSRC, name)).read()))


def test_every_kernel_is_covered():
    found = _kernels('backbone.hip')
    assert len(found) >= 6, sorted(found)                              # the pattern still reads the file
    listed = set(COVERED) | set(TIMING_HELPERS)
    assert not set(COVERED) & set(TIMING_HELPERS)
    assert found == listed, 'without a test: %s; no such kernel: %s' % (sorted(found - listed), sorted(listed - found))
    for k, ids in COVERED.items():
        assert ids, k
        for tid in ids:
            path, name = tid.split('::')
            tree = ast.parse(open(os.path.join(ROOT, path)).read())
            assert name in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, tid
    for k, caller in TIMING_HELPERS.items():                           # the named caller still reaches the helper's entry point
        entry = {'k_spin': 'frtm_spin', 'k_clock_probe': 'frtm_clock_probe'}[k]
        assert re.search(r'\b%s\s*<<<' % k, open(os.path.join(CSRC, 'backbone.hip')).read())
        assert entry in open(os.path.join(ROOT, caller)).read(), (k, caller)


def test_kernel_pattern_reads_templates_and_bounds():
    src = 'template <int V>\n__global__ __launch_bounds__(256, 4) void k_a(int x) {}\n__global__ void k_b(\n'
    assert re.findall(GLOBAL_DECL, src) == ['k_a', 'k_b']
