"""The trunk's routing decision without a GPU: frtm_backbone_conv_route (csrc/trunk_route.h: choose_route, wanted_images, kTrunkRules) on handles that
hold no weights, against the rule tables, the Winograd selection and the scanned tile restated here, at the size of the real workload (ResNet-101 on
480x854 frames: 8 and 4 frames per lane are the tracker's 16- and 8-frame batches in two lanes) -- the counts DESIGN.md quotes and no GPU test reaches,
because those use 96x160 frames."""
import ctypes
import os

import pytest

GEMM, HALO, WINO, WINO4, WINO6, BF16X3, BF16X1, S1, S2 = range(9)          # FRTM_WLAYOUT_*
TILE_G32_64x64 = 23                                                          # FRTM_TILE_G32_64x64
WINO_MIN_BLOCKS = 512                                                        # FRTM_WINO_MIN_BLOCKS
BLOCKS = {18: (2, 2, 2, 2), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}
FRAME = (480, 854)
PRECISIONS = {'fp32': (0, 0), 'bf16x3': (3, 0), 'bf16x1': (1, 0), 'bf16x1_3x3': (1, 1)}       # (bf16 pieces, the 3x3 flag)

# The rule tables of csrc/trunk_route.h (kTrunkRules), restated: shape -> fewest columns (frames x output pixels) per launch from which it is routed
RULES_BF16X3 = {(512, 2048): 3240}
RULES_BF16X1 = {(256, 1024): 1620, (1024, 256): 1620, (128, 512): 6420, (512, 128): 6420, (512, 2048): 405, (2048, 512): 3240, (256, 64): 25680}
RULES_3X3 = {(64, 64, 1): 25680, (128, 128, 1): 6420, (256, 256, 1): 12960, (512, 512, 1): 3240, (128, 128, 2): 6420, (256, 256, 2): 12960,
             (512, 512, 2): 3240, (64, 128, 2): 6420, (128, 256, 2): 1620, (256, 512, 2): 3240}


def _lib():
    from frtm_vos_amd import _hip
    return _hip.lib()


class Handle:
    """A trunk handle without weights; env: variables set around frtm_backbone_create (the only moment the library reads them)."""

    def __init__(self, arch, env=None):
        self.arch, self.bb = arch, ctypes.c_void_p()
        old = {k: os.environ.get(k) for k in env or {}}
        os.environ.update(env or {})
        try:
            assert _lib().frtm_backbone_create(arch, ctypes.byref(self.bb)) == 0
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        _lib().frtm_backbone_destroy(self.bb)

    def mode(self, name):
        pieces, flag = PRECISIONS[name]
        assert _lib().frtm_backbone_set_bf16_pieces(self.bb, pieces) == 0 and _lib().frtm_backbone_set_bf16x1_3x3(self.bb, flag) == 0

    def convs(self, H=FRAME[0], W=FRAME[1]):
        """[(idx, (Cout, Cin, k, stride, pad), (Hin, Win))] in forward order, the input sizes from the topology (torchvision v1.5: a bottleneck's stride
        sits on its 3x3): the stem at the frame, then per block conv1 [conv2] [conv3] [downsample]; the first block of stages 1..3 reads the previous
        stage's map, and only its strided conv and its downsample leave it."""
        L, info = _lib(), (ctypes.c_int * 6)()
        shapes = []
        for i in range(L.frtm_backbone_num_convs(self.bb)):
            assert L.frtm_backbone_conv_info(self.bb, i, info) == 0
            shapes.append(tuple(info[:5]))
        half = lambda hw: ((hw[0] + 1) // 2, (hw[1] + 1) // 2)          # noqa: E731  (every stride-2 step of the trunk, the max pool included)
        out, i, cur = [(0, shapes[0], (H, W))], 1, half(half((H, W)))
        for s, nb in enumerate(BLOCKS[self.arch]):
            for b in range(nb):
                own = half(cur) if (s > 0 and b == 0) else cur
                nconv = 3 if self.arch >= 50 else 2
                strided = 1 if self.arch >= 50 else 0                      # position of the conv that carries the stride
                for j in range(nconv):
                    out.append((i, shapes[i], cur if j <= strided else own))
                    i += 1
                if b == 0 and (s > 0 or self.arch >= 50):                  # downsample
                    assert shapes[i][2] == 1 and shapes[i][0] == (64 << s) * (4 if self.arch >= 50 else 1), shapes[i]
                    out.append((i, shapes[i], cur))
                    i += 1
                cur = own
        assert i == len(shapes)
        return out

    def route(self, idx, B, hw):
        out3 = (ctypes.c_int * 3)()
        assert _lib().frtm_backbone_conv_route(self.bb, idx, B, hw[0], hw[1], out3) == 0, _lib().frtm_last_error()
        return tuple(out3)


def cdiv(a, b):
    return -(-a // b)


def expected_layout(shape, B, hw, mode='fp32', min_cols=None, wino=True, wino4=2, planned=False, min_tiles=256):
    """The layout of one launch, restated from the documented order: the bf16 3x3 route, F(6x6) / F(4x4) (whichever has fewer products, each only
    where its products fill min_tiles 64x64 tiles, its tiles waste < 25 % on the map's edge and its tensors stay below 2^31 bytes), fused F(2x2) from
    512 output blocks on, bf16x3, bf16x1, the direct form.  A planned conv stays fp32."""
    cout, cin, k, s, pad = shape
    ho, wo = (hw[0] + 2 * pad - k) // s + 1, (hw[1] + 2 * pad - k) // s + 1
    cols = B * ho * wo
    if k == 3 and pad == 1 and s in (1, 2):
        need = min_cols if min_cols is not None else RULES_3X3.get((cin, cout, s))
        if mode == 'bf16x1_3x3' and not planned and need is not None and cols >= need:
            return S1 if s == 1 else S2
        if s == 1 and wino:
            best = None
            if wino4 and cin >= 128 and cin % 32 == 0 and cout % 64 == 0:
                for m in ((6, 4) if wino4 == 2 else (4,)):
                    th, tw, NP = cdiv(ho, m), cdiv(wo, m), (m + 2) ** 2
                    Tp = cdiv(B * th * tw, 64) * 64
                    if cdiv(cout, 64) * (NP * Tp // 64) < min_tiles or m * m * th * tw * 4 > 5 * ho * wo or NP * max(cin, cout) * Tp * 4 >= 0x7fffffff:
                        continue
                    if best is None or NP * Tp < best[1]:
                        best = (m, NP * Tp)
            if best:
                return WINO6 if best[0] == 6 else WINO4
            if B * cdiv(ho, 8) * cdiv(wo, 8) * cdiv(cout, 32) >= WINO_MIN_BLOCKS:
                return WINO
        return HALO
    if k == 1 and s == 1 and pad == 0 and cin % 16 == 0 and not planned:
        if mode == 'bf16x3' and cols >= RULES_BF16X3.get((cin, cout), 1 << 62):
            return BF16X3
        need = min_cols if min_cols is not None else RULES_BF16X1.get((cin, cout))
        if mode in ('bf16x1', 'bf16x1_3x3') and need is not None and cols >= need:
            return BF16X1
    return GEMM


def census(h, B, hw=FRAME, **kw):
    """{layout: launches} of one lane of B frames; every conv's layout must be the restated one, and its FLOP slot the one of its form."""
    n = {}
    for idx, shape, size in h.convs(*hw):
        lay, tile, slot = h.route(idx, B, size)
        assert lay == expected_layout(shape, B, size, **kw), (idx, shape, size, B, kw, lay)
        assert slot == {WINO: 1, WINO4: 2, WINO6: 3}.get(lay, 0), (idx, lay, slot)
        n[lay] = n.get(lay, 0) + 1
    return n


@pytest.fixture(scope='module')
def rn101():
    with Handle(101) as h:
        yield h


def test_default_tables_at_the_workload_size(rn101):
    """The counts of DESIGN.md section 4, per lane.  Derivation, ResNet-101 (3, 4, 23, 3 blocks), stage maps of 25680, 6420, 1620, 405 pixels: at 8
    frames every bf16x1 rule holds -- conv3 of 23 + 4 + 3 blocks and conv1 of every block but a stage's first (22 + 3 + 2 + 2; layer1's 64 -> 256 conv3
    is in no rule) = 59; every 3x3 rule holds: 3 + 3 + 22 + 2 = 30 stride-1 convs and the 3 openers.  At 4 frames the 256- and 512-channel 3x3 rules
    (12960 / 3240 columns) fail: 3 + 3 = 6 and layer2's opener."""
    rn101.mode('bf16x1_3x3')
    n = census(rn101, 8, mode='bf16x1_3x3')
    assert (n.get(BF16X1), n.get(S1), n.get(S2), n.get(BF16X3)) == (59, 30, 3, None), n
    n = census(rn101, 4, mode='bf16x1_3x3')
    assert (n.get(S1), n.get(S2)) == (6, 1), n
    rn101.mode('bf16x1')
    n = census(rn101, 8, mode='bf16x1')
    assert (n.get(BF16X1), n.get(S1), n.get(S2), n.get(BF16X3)) == (59, None, None, None), n
    rn101.mode('bf16x3')
    n = census(rn101, 8, mode='bf16x3')
    assert (n.get(BF16X3), n.get(BF16X1), n.get(S1), n.get(S2)) == (3, None, None, None), n
    on5 = [shape for idx, shape, size in rn101.convs() if rn101.route(idx, 8, size)[0] == BF16X3]
    assert on5 == [(2048, 512, 1, 1, 0)] * 3
    assert BF16X3 not in census(rn101, 1, mode='bf16x3')
    rn101.mode('fp32')
    n = census(rn101, 8)
    assert not set(n) & {BF16X3, BF16X1, S1, S2} and sum(n.values()) == 104, n


def test_default_tables_resnet18():
    with Handle(18) as h:
        h.mode('bf16x1_3x3')
        n = census(h, 8, mode='bf16x1_3x3')
        assert (n.get(S1), n.get(S2), n.get(BF16X1)) == (13, 3, None), n
        h.mode('bf16x1')                                      # a BasicBlock trunk has no stride-1 1x1 conv
        assert not set(census(h, 8, mode='bf16x1')) & {BF16X3, BF16X1, S1, S2}


# the seven 3x3 shapes of ResNet-101 -> the `form` column of profiles/bf16x1_trunk3x3_time.txt (recorded GPU runs), the same at 1 and at 8 frames
RECORDED_FORMS = {(64, 64, 1): WINO, (128, 128, 1): WINO6, (256, 256, 1): WINO6, (512, 512, 1): WINO4, (128, 128, 2): HALO, (256, 256, 2): HALO,
                  (512, 512, 2): HALO}


def _convs3x3(h):
    return [(idx, shape, size) for idx, shape, size in h.convs() if shape[2] == 3]


@pytest.mark.parametrize('B', (1, 8))
def test_fp32_forms_are_the_recorded_ones(rn101, B):
    L = _lib()
    rn101.mode('fp32')
    seen = set()
    for idx, shape, size in _convs3x3(rn101):
        assert rn101.route(idx, B, size)[0] == RECORDED_FORMS[(shape[1], shape[0], shape[3])], (shape, B)
        seen.add((shape[1], shape[0], shape[3]))
    assert seen == set(RECORDED_FORMS)
    try:
        assert L.frtm_backbone_set_winograd4(rn101.bb, 1) == 0                  # F(4x4) only: it passes its tests on all three wide maps
        for idx, shape, size in _convs3x3(rn101):
            want = {WINO6: WINO4}.get(RECORDED_FORMS[(shape[1], shape[0], shape[3])], RECORDED_FORMS[(shape[1], shape[0], shape[3])])
            assert rn101.route(idx, B, size)[0] == want == expected_layout(shape, B, size, wino4=1), (shape, B)
        assert L.frtm_backbone_set_winograd4(rn101.bb, 0) == 0                  # no three-launch form: fused F(2x2) where the launch has 512 blocks
        for idx, shape, size in _convs3x3(rn101):
            lay = rn101.route(idx, B, size)[0]
            assert lay == expected_layout(shape, B, size, wino4=0) and lay in (WINO, HALO), (shape, B)
            if shape[3] == 1 and B == 8:
                assert lay == WINO, shape
        assert L.frtm_backbone_set_winograd4(rn101.bb, 2) == 0 and L.frtm_backbone_set_winograd(rn101.bb, 0) == 0
        for idx, shape, size in _convs3x3(rn101):
            assert rn101.route(idx, B, size)[0] == HALO, (shape, B)
    finally:
        L.frtm_backbone_set_winograd4(rn101.bb, 2)
        L.frtm_backbone_set_winograd(rn101.bb, 1)


def test_a_planned_conv_stays_fp32(rn101):
    L = _lib()
    convs = rn101.convs()
    picks = [next(c for c in convs if c[1][:4] == want) for want in ((1024, 256, 1, 1), (256, 256, 3, 1), (256, 256, 3, 2), (2048, 512, 1, 1))]
    try:
        for idx, shape, size in picks:
            assert L.frtm_backbone_set_conv_plan(rn101.bb, idx, 1, 0) == 0
        for mode in PRECISIONS:
            rn101.mode(mode)
            for idx, shape, size in picks:
                lay, tile, _ = rn101.route(idx, 8, size)
                assert lay == expected_layout(shape, 8, size, mode=mode, planned=True) and lay <= WINO6 and tile == 1, (mode, shape, lay, tile)
            census_rest = [rn101.route(i, 8, sz)[0] for i, sh, sz in convs if i not in [p[0] for p in picks]]
            if mode == 'bf16x1_3x3':
                assert (census_rest.count(BF16X1), census_rest.count(S1), census_rest.count(S2)) == (57, 29, 2)
    finally:
        for idx, _, _ in picks:
            L.frtm_backbone_set_conv_plan(rn101.bb, idx, 0, 0)
        rn101.mode('fp32')


def test_scanned_tile(rn101):
    """256 -> 1024 (layer3's conv3) with 96..130 column tiles of 64 and Ho x Wo % 4 == 0 takes the 32x32-MFMA tile; outside, or on a map the 16-byte
    staging cannot take, the planner's choice (0)."""
    rn101.mode('fp32')
    idx = next(i for i, shape, _ in rn101.convs() if shape[:4] == (1024, 256, 1, 1))
    for B, hw, want in ((1, (80, 80), TILE_G32_64x64), (1, (64, 96), TILE_G32_64x64), (1, (80, 104), TILE_G32_64x64), (4, (30, 54), TILE_G32_64x64),
                        (1, (76, 80), 0), (1, (92, 92), 0), (1, (81, 81), 0), (8, (30, 54), 0), (1, (30, 54), 0)):
        tiles = cdiv(B * hw[0] * hw[1], 64)
        assert (96 <= tiles <= 130 and hw[0] * hw[1] % 4 == 0) == bool(want), (B, hw, tiles)          # (the cases are what they claim to be)
        assert rn101.route(idx, B, hw) == (GEMM, want, 0), (B, hw, tiles)
    other = next(i for i, shape, _ in rn101.convs() if shape[:4] == (256, 1024, 1, 1))
    assert rn101.route(other, 1, (80, 80)) == (GEMM, 0, 0)


def test_min_cols_override_reaches_layouts_6_7_8_only():
    """FRTM_BF16X1_MIN_COLS=0, read when the handle is created: every eligible conv on its bf16x1 layout at any size; the bf16x3 rule is not touched."""
    for arch in (50, 18):
        with Handle(arch, env={'FRTM_BF16X1_MIN_COLS': '0'}) as h:
            h.mode('bf16x1_3x3')
            n = census(h, 1, hw=(96, 160), mode='bf16x1_3x3', min_cols=0)
            for idx, shape, size in h.convs(96, 160):
                cout, cin, k, s, pad = shape
                lay = h.route(idx, 1, size)[0]
                if k == 1 and s == 1 and cin % 16 == 0:
                    assert lay == BF16X1, shape
                elif k == 3:
                    assert lay == (S1 if s == 1 else S2), shape
                else:
                    assert lay == GEMM, shape                     # the stem and the strided downsamples
            assert BF16X3 not in n and n.get(S1) == 13 and n.get(S2) == 3 and n.get(BF16X1, 0) == (33 if arch == 50 else 0), n
            h.mode('bf16x3')
            assert not set(census(h, 1, hw=(96, 160), mode='bf16x3', min_cols=0)) & {BF16X3, BF16X1, S1, S2}
            assert census(h, 8, mode='bf16x3', min_cols=0).get(BF16X3) == (3 if arch == 50 else None)
    with Handle(50) as h:                                         # the variable is gone again: the table decides
        h.mode('bf16x1_3x3')
        assert not set(census(h, 1, hw=(96, 160), mode='bf16x1_3x3')) & {BF16X3, BF16X1, S1, S2}


def test_bad_arguments(rn101):
    L = _lib()
    out3 = (ctypes.c_int * 3)()
    n = L.frtm_backbone_num_convs(rn101.bb)
    for args in ((None, 0, 1, 480, 854, out3), (rn101.bb, n, 1, 480, 854, out3), (rn101.bb, -1, 1, 480, 854, out3), (rn101.bb, 0, 0, 480, 854, out3),
                 (rn101.bb, 0, 1, 0, 854, out3), (rn101.bb, 0, 1, 480, 854, None)):
        assert L.frtm_backbone_conv_route(*args) == -1, args[1:5]
        assert b'frtm_backbone_conv_route' in L.frtm_last_error()
