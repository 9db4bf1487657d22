"""The trunk's stem (csrc/backbone.hip: k_normalize_u8 -> 7x7 stride-2 conv + BN + ReLU -> k_maxpool3s2_x4 / k_maxpool3s2) stated twice.

stem_exact: with DELTA weights -- output channel m holds one 1.0 at (c_m, ky_m, kx_m) --, BN folded to scale 1 / shift 0 and the
normalisation set to scale 1 / bias 0, layer1 is an integer function of the uint8 frame: every conv output is one product 1 * pixel plus
zeros (exact in fp32 in any accumulation order), ReLU leaves values >= 0 alone and max is exact.  The GPU tests
(tests/test_trunk_stem_gpu.py) compare with torch.equal; tests/test_trunk_stem.py holds this statement to F.conv2d + F.max_pool2d at float64.

    pad  = the frame with 3 zeros around it
    conv[m, oy, ox] = pad[c_m, 2 oy + ky_m, 2 ox + kx_m],   h1 = (H + 1) // 2, w1 = (W + 1) // 2
    out[m, py, px]  = max of conv[m, 2 py - 1 .. 2 py + 1, 2 px - 1 .. 2 px + 1] inside the map,   Hp = (h1 + 1) // 2, Wp = (w1 + 1) // 2

stem_fp: the first three lines of oracle/cpu_ref.py: resnet_forward at a given dtype (real weights, ImageNet normalisation).

branch_classes: which branches of the three kernels a (H, W, B) reaches, restated from their conditions (not their code), so that the
CPU test can say that SIZES and WIDE together reach every one."""
import torch
import torch.nn.functional as F

TAPS = [(c, ky, kx) for c in range(3) for ky in range(7) for kx in range(7)]               # all 147
_EDGE = [(0, 0), (0, 6), (6, 0), (6, 6), (3, 3)]                                             # four corners and the centre


def _tap_set(c):
    """64 taps: the 49 of plane c, then the corner and centre taps of the other two planes (10, repeated to fill 15 channels)."""
    other = [(o, ky, kx) for o in range(3) if o != c for ky, kx in _EDGE]
    return [(c, ky, kx) for ky in range(7) for kx in range(7)] + [other[i % len(other)] for i in range(15)]


TAP_SETS = [_tap_set(c) for c in range(3)]

SIZES = [(H, W) for H in range(32, 44) for W in range(33, 49)]                               # 192; the entry refuses frames below 32
WIDE = (8, 334, 1031)                                                                        # (B, H, W): 2,121,600 quads > 8192 * 256 threads; Wo = 258
KINDS = ('random', 'bright', 'dark')
RING = 4

TAIL_CLASSES = ['tail r=%d %s right' % (r, s) for r in (1, 2, 3) for s in ('with', 'without')] + ['tail r=4 without right']
ALL_CLASSES = (['full'] + TAIL_CLASSES + ['w1 odd', 'w1 even', 'h1 odd', 'h1 even'] + ['Ho%%4=%d' % i for i in range(4)]
               + ['(W+6)%%4=%d' % i for i in range(4)] + ['x4 second x block', 'v1 second x block', 'grid-stride loop'])
WIDE_ONLY = ['x4 second x block', 'v1 second x block', 'grid-stride loop']


def frame(kind, H, W, seed):
    """(3, H, W) uint8.  'random': uniform bytes.  'bright': the outer RING pixels 255 around 0..127 -- a missed edge column or row lowers
    a maximum.  'dark': the outer RING pixels 1 around 128..255 -- a window one column too wide, or a border that is not zero, raises or
    changes one."""
    g = torch.Generator().manual_seed(seed)
    if kind == 'random':
        return torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g)
    lo, hi, ring = (0, 128, 255) if kind == 'bright' else (128, 256, 1)
    img = torch.full((3, H, W), ring, dtype=torch.uint8)
    img[:, RING:H - RING, RING:W - RING] = torch.randint(lo, hi, (3, H - 2 * RING, W - 2 * RING), dtype=torch.uint8, generator=g)
    return img


def frames(i, H, W, B=2):
    """B frames for the i-th shape of a loop: kinds rotate, so that over any three consecutive shapes every kind occurs at every position."""
    return torch.stack([frame(KINDS[(i + b) % 3], H, W, 1000 * i + b) for b in range(B)])


def out_size(H, W):
    h1, w1 = (H + 1) // 2, (W + 1) // 2
    return (h1 + 1) // 2, (w1 + 1) // 2


def delta_weights(taps, dtype=torch.float32):
    w = torch.zeros(len(taps), 3, 7, 7, dtype=dtype)
    for m, (c, ky, kx) in enumerate(taps):
        w[m, c, ky, kx] = 1
    return w


def stem_exact(img_u8, taps):
    """(B, 3, H, W) or (3, H, W) uint8 -> (B, len(taps), Hp, Wp) int64, in integer arithmetic only."""
    img = torch.as_tensor(img_u8)
    if img.dim() == 3:
        img = img.unsqueeze(0)
    B, _, H, W = img.shape
    h1, w1 = (H + 1) // 2, (W + 1) // 2
    Hp, Wp = (h1 + 1) // 2, (w1 + 1) // 2
    pad = torch.zeros(B, 3, H + 6, W + 6, dtype=torch.int64)
    pad[:, :, 3:3 + H, 3:3 + W] = img.to(torch.int64)
    outside = torch.iinfo(torch.int64).min                             # -inf of the pool
    conv = torch.full((B, len(taps), h1 + 2, w1 + 2), outside, dtype=torch.int64)
    for m, (c, ky, kx) in enumerate(taps):
        conv[:, m, 1:1 + h1, 1:1 + w1] = pad[:, c, ky:ky + 2 * h1 - 1:2, kx:kx + 2 * w1 - 1:2]
    inner = conv[:, :, 1:1 + h1, 1:1 + w1]
    inner.clamp_(min=0)                                                # ReLU: nothing to do on bytes, stated all the same
    out = torch.full((B, len(taps), Hp, Wp), outside, dtype=torch.int64)
    for dy in range(3):
        for dx in range(3):
            out = torch.maximum(out, conv[:, :, dy:dy + 2 * Hp - 1:2, dx:dx + 2 * Wp - 1:2])
    return out


def stem_fp(img_u8, P, dtype):
    """oracle/cpu_ref.py: resnet_forward up to the first tap, at ``dtype`` -> {'layer1': (B, 64, Hp, Wp)}."""
    img = torch.as_tensor(img_u8)
    if img.dim() == 3:
        img = img.unsqueeze(0)
    p = {k: P[k].to(dtype) for k in ('conv1.weight', 'bn1.running_mean', 'bn1.running_var', 'bn1.weight', 'bn1.bias')}
    stds = torch.tensor((0.229, 0.224, 0.225), dtype=dtype).reshape(1, 3, 1, 1)
    means = torch.tensor((0.485, 0.456, 0.406), dtype=dtype).reshape(1, 3, 1, 1)
    x = (1 / 255 / stds) * img.to(dtype) + (-means / stds)
    x = F.conv2d(x, p['conv1.weight'], stride=2, padding=3)
    x = F.relu(F.batch_norm(x, p['bn1.running_mean'], p['bn1.running_var'], p['bn1.weight'], p['bn1.bias'], training=False, eps=1e-5))
    return {'layer1': F.max_pool2d(x, 3, 2, 1)}


def branch_classes(H, W, B):
    """The classes of ALL_CLASSES that a batch of B frames of H x W reaches.  Thread t of a pooled row owns outputs ox0 = 4 t .. 4 t + 3,
    whose windows start at column x0 = 8 t of the w1-wide stem output."""
    h1, w1 = (H + 1) // 2, (W + 1) // 2
    Ho, Wo = (h1 + 1) // 2, (w1 + 1) // 2
    got = set()
    for t in range((Wo + 3) // 4):
        ox0, x0 = 4 * t, 8 * t
        if x0 + 7 < w1 and ox0 + 3 < Wo:
            got.add('full')
            continue
        r = min(4, Wo - ox0)
        right = 2 * (ox0 + r - 1) + 1 < w1                             # the last output's centre column + 1 inside the row
        got.add('tail r=%d %s right' % (r, 'with' if right else 'without'))
    got.add('w1 odd' if w1 % 2 else 'w1 even')
    got.add('h1 odd' if h1 % 2 else 'h1 even')                         # odd: the bottom window is clipped
    got.add('Ho%%4=%d' % (Ho % 4))
    got.add('(W+6)%%4=%d' % ((W + 6) % 4))                             # the normaliser's tail quad
    if Wo > 256:
        got.add('x4 second x block')
    if Wo > 64:
        got.add('v1 second x block')
    if B * 3 * (H + 6) * ((W + 6 + 3) // 4) > 8192 * 256:
        got.add('grid-stride loop')
    return got


# ---- the GPU side (imported by tests/test_trunk_stem_gpu.py and by its child process) ---------------------------------------------------
def delta_trunk(taps, dev, name='resnet18', seed=1):
    """A trunk whose stem is the delta stem of ``taps``: conv 0 loaded directly with scale 1 / shift 0 (bn1's running_var + eps does not
    give exactly 1), the normalisation replaced by scale 1 / bias 0."""
    from oracle import cpu_ref as O
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    ext = ResnetFeatureExtractor(name, weights=O.resnet_random_params(name, seed)).to(dev)
    set_delta_stem(ext, taps)
    ext.norm_weight = torch.ones_like(ext.norm_weight)
    ext.norm_bias = torch.zeros_like(ext.norm_bias)
    return ext


def set_delta_stem(ext, taps):
    from frtm_vos_amd import _hip
    w = delta_weights(taps).to(ext.device).contiguous()
    scale, shift = torch.ones(64, device=ext.device), torch.zeros(64, device=ext.device)
    with torch.cuda.device(ext.device):
        _hip.call('frtm_backbone_set_conv', ext._handle, 0, _hip.ptr(w), _hip.ptr(scale), _hip.ptr(shift))
        torch.cuda.current_stream().synchronize()                      # the temporaries die with this scope


def first_difference(got, want):
    """(frame, channel, y, x, got, want) of the first differing element of two equal-shaped tensors, or None."""
    if got.shape != want.shape:
        return ('shape', tuple(got.shape), tuple(want.shape))
    bad = (got != want).nonzero()
    if not len(bad):
        return None
    b, m, y, x = (int(v) for v in bad[0])
    return (b, m, y, x, float(got[b, m, y, x]), float(want[b, m, y, x]))


def check_sizes(ext, taps, sizes, B=2, lane_set=0):
    """ext(frames)['layer1'] == stem_exact(frames) for every size, the largest first (arenas allocated once) -> list of
    (size, first difference) of the sizes that differ."""
    failed = []
    for i, (H, W) in enumerate(sorted(sizes, key=lambda s: -s[0] * s[1])):
        img = frames(i, H, W, B)
        got = ext(img.to(ext.device), ['layer1'], lane_set=lane_set)['layer1'].cpu()
        want = stem_exact(img, taps).to(torch.float32)
        if not torch.equal(got, want):
            failed.append(((H, W), first_difference(got, want)))
    return failed
