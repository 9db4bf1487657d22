"""Plain torch definitions of the first-frame augmentation kernels (csrc/image_ops.hip), one per kernel, and the cases the tests run them at.
Every function works in the dtype it is given and on the device of its arguments, so the same text serves as the float64 reference on the
CPU and as the fp32 yardstick of the gate on the GPU.  Where oracle/warp_ref.py or oracle/aug_ref.py state the operation it is called or
restated in the same order of operations; tests/test_image_refs.py asserts that the two agree exactly in float64.

A function whose kernel quantises returns the value BEFORE the quantiser as well: every filled pyramid level unfloored (pull-push), the
float value before truncation (blend), the float interpolant before rounding (uint8 warp).  The batched warps take the inverse 2x3 as
given (fp32 numbers), as the kernels do.

The three judging rules of tests/test_image_ops_gpu.py are stated here once (gate_tol, envelope, the quantisers), so that the CPU suite can
assert from the fp32 and float64 legs alone that no envelope is vacuous (LOOSE_CAP).
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle.aug_ref import gauss_blur_ref
from oracle.warp_ref import _cubic_weights, _fetch

LOOSE_CAP = 0.05          # largest share of a case's quantised outputs whose envelope may span two values

# kernel of csrc/image_ops.hip -> the functions of tests/test_image_ops_gpu.py that launch it (tests/test_image_refs.py: complete, and they exist)
KERNELS = {
    'k_warp_affine': ('test_warp_affine_exact_set', 'test_warp_affine_second_trip'),
    'k_warp_mask_batch': ('test_warp_mask_batch',),
    'k_warp_mask_batch_dev': ('test_warp_mask_batch_dev',),
    'k_warp_affine_batch': ('test_warp_affine_batch',),
    'k_blur2d': ('test_blur2d_tables', 'test_blur_gauss2d', 'test_blur_lds_limit'),
    'k_mask_stats': ('test_mask_stats',),
    'k_aug_prepare': ('test_aug_prepare',),
    'k_pp_down': ('test_pull_push_fill',),
    'k_pp_up': ('test_pull_push_fill',),
    'k_aug_transforms': ('test_aug_transforms',),
    'k_aug_blend': ('test_aug_blend_exact_alpha', 'test_aug_blend_fractional_alpha'),
    'k_label_mask': ('test_label_mask',),
}


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# the judging rules
# ---------------------------------------------------------------------------------------------------------------------------------
def gate_tol(ref64, t32):
    """The bound of the project's gate (tests/test_refiner_train_gpu.py::_gate): max(4 max|torch32 - ref64|, 1e-6 max|ref64|)."""
    r = ref64.detach().double().cpu()
    e32 = float((t32.detach().double().cpu() - r).abs().max()) if r.numel() else 0.0
    return max(4 * e32, 1e-6 * (float(r.abs().max()) if r.numel() else 0.0))


def q_floor(v):
    """The fill's finest level and the blend: clamp to [0, 255], then drop the fraction (truncation = floor on non-negative values)."""
    return v.clamp(0, 255).floor()


def q_round(v):
    """The uint8 warp: clamp to [0, 255], then round half up."""
    return (v.clamp(0, 255) + 0.5).floor()


def envelope(v64, tol, q):
    """(lo, hi, loose): the quantised values of v64 -+ tol and where they differ.  A quantised output passes where lo <= out <= hi."""
    lo, hi = q(v64 - tol), q(v64 + tol)
    return lo, hi, lo != hi


def loose_share(v64, v32, q, where=None):
    """Share of the elements (of `where`) whose envelope spans two values, from the two reference legs alone."""
    v64 = v64.double().cpu()
    loose = envelope(v64, gate_tol(v64, v32), q)[2]
    if where is not None:
        loose = loose[where]
    return float(loose.double().mean()) if loose.numel() else 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# k_mask_stats, k_aug_prepare, k_label_mask
# ---------------------------------------------------------------------------------------------------------------------------------
def mask_stats(mask):
    """frtm_mask_stats.  mask (H,W), set where > 0 -> [count, max(x + 1), max(W - x), max(y + 1), max(H - y)] over the set pixels, all 0 if none."""
    m = (mask > 0).cpu()
    Hh, Ww = m.shape
    if not bool(m.any()):
        return [0, 0, 0, 0, 0]
    ys, xs = torch.nonzero(m, as_tuple=True)
    return [int(m.sum()), int(xs.max()) + 1, Ww - int(xs.min()), int(ys.max()) + 1, Hh - int(ys.min())]


def aug_prepare(image_u8, label_u8, dtype=torch.float64):
    """frtm_aug_prepare.  image (3,H,W) uint8, label (H,W) uint8 (any value > 0 is set) -> target (4,H,W) = (image * mask, mask * 255),
    level 0 of the fill pyramid (4,H,W) = (image * known, known) with known = 1 - (mask dilated by one pixel, 3x3, clipped at the border),
    the float mask (H,W) and the {0,1} label (H,W) uint8."""
    im = image_u8.to(dtype)
    m = (label_u8 > 0).to(dtype)
    hole = F.max_pool2d(m[None, None], 3, 1, 1)[0, 0]
    known = 1 - hole
    return dict(target=torch.cat((im * m, m[None] * 255)), pyr0=torch.cat((im * known, known[None])), maskf=m, label01=(label_u8 > 0).to(torch.uint8))


def label_mask(labels_u8, obj_id):
    """frtm_label_mask -> (uint8 mask, float plane) of labels == obj_id."""
    m = labels_u8 == obj_id
    return m.to(torch.uint8), m.to(torch.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_pp_down, k_pp_up
# ---------------------------------------------------------------------------------------------------------------------------------
def pull_push_sizes(Hh, Ww):
    """Level sizes: ceil-halving while min(H, W) > 2, at most 10 levels below the image."""
    out = [(Hh, Ww)]
    while min(out[-1]) > 2 and len(out) <= 10:
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def pull_push_elems(Hh, Ww):
    return sum(4 * h * w for h, w in pull_push_sizes(Hh, Ww))


def pull_push_fill(level0, dtype=torch.float64):
    """frtm_pull_push_fill.  level0 (4,H,W) = (image * known, known) -> (levels, quantised): the pyramid as the launch leaves it, level l a
    (4,h,w) tensor of the FILLED, unfloored colour planes and the known plane of the way down (the coarsest level is never filled: its
    unknown pixels hold 0); quantised (3,H,W) = level 0's colours clamped to [0, 255] and floored, which is what the kernel stores there.
    Restates oracle.aug_ref.pull_push_fill_ref operation by operation."""
    cur, k = level0[:3].to(dtype), level0[3:4].to(dtype)
    levels = []
    n = 0
    while True:
        levels.append((cur, k))
        n += 1
        if not (min(cur.shape[-2:]) > 2 and n <= 10):
            break
        Hf, Wf = cur.shape[-2:]
        Hc, Wc = (Hf + 1) // 2, (Wf + 1) // 2
        pad = (0, 2 * Wc - Wf, 0, 2 * Hc - Hf)
        ck = F.pad(cur * k, pad).reshape(3, Hc, 2, Wc, 2)
        kk = F.pad(k, pad).reshape(1, Hc, 2, Wc, 2)
        s = ((ck[:, :, 0, :, 0] + ck[:, :, 0, :, 1]) + ck[:, :, 1, :, 0]) + ck[:, :, 1, :, 1]          # row-major window order
        kn = ((kk[:, :, 0, :, 0] + kk[:, :, 0, :, 1]) + kk[:, :, 1, :, 0]) + kk[:, :, 1, :, 1]
        inv = torch.where(kn > 0, 1.0 / kn.clamp(min=1), torch.zeros_like(kn))
        cur, k = s * inv, (kn > 0).to(dtype)
    dev = cur.device
    fill = levels[-1][0]
    filled = [None] * len(levels)
    filled[-1] = torch.cat(levels[-1])
    for li in range(len(levels) - 2, -1, -1):
        fine, kf = levels[li]
        Hf, Wf = fine.shape[-2:]
        Hc, Wc = fill.shape[-2:]
        sy, sx = torch.tensor(Hc, dtype=dtype, device=dev) / Hf, torch.tensor(Wc, dtype=dtype, device=dev) / Wf
        fy = ((torch.arange(Hf, dtype=dtype, device=dev) + 0.5) * sy - 0.5).clamp(min=0)
        fx = ((torch.arange(Wf, dtype=dtype, device=dev) + 0.5) * sx - 0.5).clamp(min=0)
        y0 = fy.floor().long().clamp(max=Hc - 1)
        x0 = fx.floor().long().clamp(max=Wc - 1)
        y1, x1 = (y0 + 1).clamp(max=Hc - 1), (x0 + 1).clamp(max=Wc - 1)
        ly, lx = (fy - y0.to(dtype)).view(1, -1, 1), (fx - x0.to(dtype)).view(1, 1, -1)
        g = lambda yy, xx: fill[:, yy][:, :, xx]
        up = (1 - ly) * ((1 - lx) * g(y0, x0) + lx * g(y0, x1)) + ly * ((1 - lx) * g(y1, x0) + lx * g(y1, x1))
        fill = torch.where(kf > 0, fine, up)
        filled[li] = torch.cat((fill, kf))
    return filled, fill.clamp(0, 255).floor()


# hole patterns of the fill cases: name -> known plane (H,W) {0,1}
def hole_pattern(name, Hh, Ww):
    known = torch.ones(Hh, Ww)
    if name == 'block':
        known[Hh // 3:max(Hh // 3 + 1, 2 * Hh // 3), Ww // 3:max(Ww // 3 + 1, 2 * Ww // 3)] = 0
    elif name == 'top_right':
        known[:max(1, Hh // 4)] = 0
        known[:, Ww - max(1, Ww // 4):] = 0
    elif name == 'corner_only':
        known[:] = 0
        known[Hh - 1, 0] = 1
    elif name == 'nothing_known':
        known[:] = 0
    elif name == 'random90':
        known = (torch.rand(Hh, Ww, generator=gen(Hh, Ww, 90)) >= 0.9).float()
    else:
        raise ValueError(name)
    return known


PP_SMALL = [(2, 7), (3, 3), (5, 9), (17, 33), (37, 53), (64, 64), (65, 129), (100, 3)]
PP_LARGE = (1030, 1030)          # more than 1024 * 256 coarse and 2048 * 256 fine pixels: the second trips of both kernels
PP_PATTERNS = ('block', 'top_right', 'corner_only', 'nothing_known')
PP_CASES = [(h, w, p) for h, w in PP_SMALL for p in PP_PATTERNS + ('random90',)] + [(PP_LARGE[0], PP_LARGE[1], p) for p in PP_PATTERNS]


def pull_push_image(Hh, Ww, integer=False):
    """The image of the fill cases, (3,H,W) float.  Values k + f with f in [0.25, 0.75]: the smallest pyramids copy known values into the
    hole unchanged (a clamped border tap, a window with one known pixel), and a copy of an INTEGER sits exactly on the step of the floor,
    where an envelope of any width spans two values.  integer=True: f = 0, the values frtm_aug_prepare leaves."""
    g = gen(Hh, Ww, 7)
    im = torch.randint(0, 256, (3, Hh, Ww), generator=g).float()
    return im if integer else im + 0.25 + 0.5 * torch.rand(3, Hh, Ww, generator=g)


def pull_push_level0(Hh, Ww, pattern, integer=False):
    """Level 0 as frtm_aug_prepare lays it out: image times known, and known."""
    known = hole_pattern(pattern, Hh, Ww)
    return torch.cat((pull_push_image(Hh, Ww, integer) * known, known[None]))


# ---------------------------------------------------------------------------------------------------------------------------------
# k_blur2d
# ---------------------------------------------------------------------------------------------------------------------------------
def gauss_table(half, qa, qb, qc, dtype=torch.float64, device='cpu'):
    """The normalised table of frtm_blur_gauss2d, as oracle.aug_ref.gauss_blur_ref forms it."""
    r = torch.arange(-half, half + 1, dtype=dtype, device=device)
    yy, xx = torch.meshgrid(r, r, indexing='ij')
    g = torch.exp(-0.5 * (qa * xx * xx + 2 * qb * xx * yy + qc * yy * yy))
    return g / g.sum()


def blur2d(x, G, dtype=torch.float64):
    """frtm_blur2d.  x (P,H,W), G (kh,kw) odd sizes: cross-correlation with zero padding, out[y,x] = sum_ij G[i,j] x[y + i - kh//2, x + j - kw//2],
    as shifted products summed in row-major tap order (elementwise operations only)."""
    kh, kw = G.shape
    Hh, Ww = x.shape[-2:]
    xp = F.pad(x.to(dtype), (kw // 2, kw // 2, kh // 2, kh // 2))
    G = G.to(dtype)
    out = torch.zeros(x.shape, dtype=dtype, device=x.device)
    for i in range(kh):
        for j in range(kw):
            out = out + G[i, j] * xp[:, i:i + Hh, j:j + Ww]
    return out


def blur_gauss2d(x, half, qa, qb, qc, dtype=torch.float64, taps=False):
    """frtm_blur_gauss2d.  The definition is oracle.aug_ref.gauss_blur_ref (taps=False: called as it stands); taps=True is the same operation
    through blur2d, for the fp32 leg on the GPU, where F.conv2d would go through MIOpen."""
    if taps:
        return blur2d(x, gauss_table(half, qa, qb, qc, dtype, x.device), dtype)
    return gauss_blur_ref(x, ('gauss', half, qa, qb, qc), dtype)


def blur_spec(blur_size, angle_deg):
    """(half, qa, qb, qc) as ImageAugmenter._blur_spec forms them (model/augmenter.py), restated so that the CPU suite needs no product import."""
    b = np.deg2rad(angle_deg)
    R = np.array([[np.cos(b), np.sin(b)], [-np.sin(b), np.cos(b)]])
    icov = np.linalg.inv(R @ np.diag((blur_size, 0.1)) @ R.T)
    half = int(blur_size / 2 + 0.5)
    half = half + (half + 1) % 2
    return int(half), float(icov[0, 0]), float(0.5 * (icov[0, 1] + icov[1, 0])), float(icov[1, 1])


BLUR_IMAGES = [(1, 1), (15, 17), (16, 16), (33, 47)]
BLUR_TABLES = [(1, 1), (1, 7), (9, 3), (17, 17)]          # 17 x 17 = 289 taps: the second trip of the table load
BLUR_Q = [blur_spec(bs, ang)[1:] for bs in (1.0, 2.0, 5.0) for ang in (0, 45, 90, 135)] + [(1 / 400.0, 0.0, 1 / 400.0)]   # the last: isotropic, sigma 20
BLUR_HALVES = [0, 1, 3, 8, 40]          # 1 and 3 are the product's; 40 is the largest whose tile fits


# ---------------------------------------------------------------------------------------------------------------------------------
# k_warp_affine, k_warp_mask_batch(_dev), k_warp_affine_batch
# ---------------------------------------------------------------------------------------------------------------------------------
MODES = ('nearest', 'bilinear', 'bicubic')          # the C side's mode 0, 1, 2


def invert32(fwd6):
    """invert_affine of csrc/image_ops.hip: the inverse 2x3 of a forward 2x3 in fp32 arithmetic; None where the fp32 determinant is 0."""
    a, b, tx, c, d, ty = (np.float32(v) for v in np.asarray(fwd6, dtype=np.float32).ravel()[:6])
    det = a * d - b * c
    if det == 0:
        return None
    return np.array([d / det, -b / det, (b * ty - d * tx) / det, -c / det, a / det, (c * tx - a * ty) / det], dtype=np.float32)


def source_coords(inv6, size, dtype=torch.float64, device='cpu'):
    """(sx, sy) (Hd,Wd): sx = m0 x + m1 y + m2, sy = m3 x + m4 y + m5 with the inverse's numbers as given."""
    m = [torch.tensor(float(v), dtype=dtype, device=device) for v in np.asarray(inv6).ravel()[:6]]
    ys, xs = torch.meshgrid(torch.arange(size[0], dtype=dtype, device=device), torch.arange(size[1], dtype=dtype, device=device), indexing='ij')
    return m[0] * xs + m[1] * ys + m[2], m[3] * xs + m[4] * ys + m[5]


def warp_affine(src, inv6, size, mode, dtype=torch.float64):
    """frtm_warp_affine(_u8) with the inverse given.  src (C,Hs,Ws) float or uint8 -> the float interpolant (C,Hd,Wd), before any rounding.
    oracle.warp_ref.warp_affine_ref from its inverse on, operation by operation."""
    s = src.to(dtype)
    sx, sy = source_coords(inv6, size, dtype, src.device)
    if mode == 'nearest':
        return _fetch(s, torch.floor(sy + 0.5).long(), torch.floor(sx + 0.5).long())
    x0, y0 = torch.floor(sx), torch.floor(sy)
    if mode == 'bilinear':
        fx, fy = sx - x0, sy - y0
        x0, y0 = x0.long(), y0.long()
        return ((1 - fy) * ((1 - fx) * _fetch(s, y0, x0) + fx * _fetch(s, y0, x0 + 1)) +
                fy * ((1 - fx) * _fetch(s, y0 + 1, x0) + fx * _fetch(s, y0 + 1, x0 + 1)))
    assert mode == 'bicubic', mode
    wx, wy = _cubic_weights(sx - x0), _cubic_weights(sy - y0)
    x0, y0 = x0.long(), y0.long()
    out = torch.zeros(s.shape[0], int(size[0]), int(size[1]), dtype=dtype, device=src.device)
    for j in range(4):
        row = torch.zeros_like(out)
        for k in range(4):
            row = row + wx[k] * _fetch(s, y0 - 1 + j, x0 - 1 + k)
        out = out + wy[j] * row
    return out


def round_u8(v):
    """The uint8 result of a warp: round half up, saturate (oracle.warp_ref.warp_affine_ref's last line)."""
    return torch.floor(v + 0.5).clamp(0, 255).to(torch.uint8)


def warp_mask_batch(src, inv, size, dtype=torch.float64):
    """frtm_warp_mask_batch(_dev).  src (Hs,Ws) float, inv (n,6) -> ((n,Hd,Wd) uint8 {0,1}: nearest pick > 0, [set pixels per plane])."""
    planes = torch.stack([(warp_affine(src[None], m, size, 'nearest', dtype)[0] > 0).to(torch.uint8) for m in np.asarray(inv).reshape(-1, 6)])
    return planes, [int(p.sum()) for p in planes]


def warp_affine_batch(src, inv, index, n, size, dtype=torch.float64):
    """frtm_warp_affine_batch.  src (C,Hs,Ws), inv (m,6), index: n entries into inv, or None (then j itself) -> (n,C,Hd,Wd) bicubic, clamped to [0, 255]."""
    inv = np.asarray(inv).reshape(-1, 6)
    return torch.stack([warp_affine(src, inv[j if index is None else int(index[j])], size, 'bicubic', dtype).clamp(0, 255) for j in range(n)])


def exact_transforms(Hs, Ws, Hd, Wd):
    """The exact-transform set: (name, forward 2x3 float32) with entries in {0, +-0.5, +-1, +-2}, a power of two as determinant and
    translations that are multiples of 0.25, so that the fp32 inversion and every source coordinate are exact and the kernel and the float64
    reference pick the same taps."""
    M = lambda a, b, tx, c, d, ty: np.array([a, b, tx, c, d, ty], dtype=np.float32)
    return [
        ('identity', M(1, 0, 0, 0, 1, 0)),
        ('shift_int', M(1, 0, 2, 0, 1, -1)),
        ('shift_half', M(1, 0, 0.5, 0, 1, 0.5)),                 # every nearest pick on the half-integer tie
        ('shift_quarter', M(1, 0, 0.25, 0, 1, -0.75)),
        ('flip_lr', M(-1, 0, Ws - 1, 0, 1, 0)),
        ('rot90', M(0, -1, Hs - 1, 1, 0, 0)),
        ('scale2', M(2, 0, 0, 0, 2, 1)),                          # source coordinates k / 2
        ('scale_half', M(0.5, 0, 0, 0, 0.5, 0.25)),
        ('shear_b', M(1, 0.5, 0, 0, 1, 0)),
        ('shear_c', M(1, 0, 0, 0.5, 1, 0)),
        ('one_row_one_column', M(1, 0, Wd - 1, 0, 1, Hd - 1)),   # only source row 0 and column 0 reach the destination
        ('nothing_inside', M(1, 0, Wd + 2, 0, 1, 0)),             # beyond the bicubic taps too: every output is 0
    ]


WARP_SIZES = [((5, 7), (9, 4)), ((33, 47), (20, 61)), ((1, 1), (3, 3))]
WARP_LARGE = ((300, 301), (600, 600), 3, 'scale2')          # C * Hd * Wd = 1 080 000 > 4096 * 256: the second trip of k_warp_affine


def warp_source_f32(C, Hs, Ws):
    """Float source planes with values beyond both ends of [0, 255] (so the clamp of the batched warp binds at both ends)."""
    return torch.randn(C, Hs, Ws, generator=gen(C, Hs, Ws, 3)) * 120 + 128


def _blocks_u8(s):
    """A block of 255 (two wide at least: the interpolant half-way between two 255s exceeds 255) next to blocks of 1 (not 0: half-way across
    an edge between 255 and 0 the interpolant is 127.5, on the tie), one pixel inside the border for the same reason (the zero padding), and a
    0 in the far corner."""
    Hs, Ws = s.shape[-2:]
    h, w = max(2, Hs // 3), max(2, Ws // 4)
    s[..., 1:1 + h, 1:1 + w] = 255
    s[..., 1:1 + h, 1 + w:1 + 2 * w] = 1
    s[..., 1 + h, 1:1 + w] = 1
    s[..., -1, -1] = 0
    return s


@functools.lru_cache(maxsize=None)
def _small_plane_u8(Hs, Ws, c):
    """Plane c of a source of fewer than 100 pixels: one loose element of a 9 x 4 destination is 2.8 % of the launch, so chance ties are kept
    out -- the plane is the c-th draw (seeds 0, 1, ...) none of whose float64 bicubic interpolants, under the exact-transform set to the
    destination WARP_SIZES pairs with this source, lies within 1e-3 of a rounding tie.  The criterion reads the reference alone."""
    size = dict(WARP_SIZES)[(Hs, Ws)]
    found = 0
    for seed in range(1000):
        s = _blocks_u8(torch.randint(0, 256, (1, Hs, Ws), generator=gen(Hs, Ws, 5, seed)))
        if all(float(((warp_affine(s, invert32(f), size, 'bicubic') % 1) - 0.5).abs().min()) > 1e-3 for _, f in exact_transforms(Hs, Ws, *size)):
            found += 1
            if found > c:
                return s[0].to(torch.uint8)
    raise AssertionError('no tie-free plane among 1000 draws')


def warp_source_u8(C, Hs, Ws, mode):
    """uint8 source planes of a mode, chosen so that few float interpolants under the exact-transform set sit exactly ON the rounding tie
    v = k + 0.5, where an envelope of any width spans two values.  The set puts source coordinates on multiples of 1/4.
    bilinear: weights are multiples of 1/16, so multiples of 16 (0 .. 240) give integers; a random uint8 source would put a quarter of
    the outputs of a half-pixel shift on the tie.  One pixel: 240.
    nearest, bicubic: random values with the blocks of _blocks_u8, so that the bicubic overshoot saturates at both ends; the
    cubic weights at half a pixel are (-3, 19, 19, -3) / 32, which puts 1 / 32 of such outputs on the tie and multiples of 16 every second
    one.  One pixel: 255 (odd, like every numerator of the weights: no product is an odd multiple of 1/2)."""
    if mode == 'bilinear':
        s = torch.randint(0, 16, (C, Hs, Ws), generator=gen(C, Hs, Ws, 4)) * 16
        if Hs * Ws == 1:
            s[:] = 240
    elif 1 < Hs * Ws < 100:
        return torch.stack([_small_plane_u8(Hs, Ws, c) for c in range(C)])
    else:
        s = torch.randint(0, 256, (C, Hs, Ws), generator=gen(C, Hs, Ws, 5))
        if Hs * Ws > 1:
            _blocks_u8(s)
        else:
            s[:] = 255
    return s.to(torch.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_aug_blend, k_aug_transforms
# ---------------------------------------------------------------------------------------------------------------------------------
def aug_blend(wt, canvas, cand_labels, index, dtype=torch.float64):
    """frtm_aug_blend.  wt (n,4,H,W), canvas (n,3,H,W), cand_labels (m,H,W) uint8, index (n,) -> (v (n,3,H,W): target * alpha + canvas * (1 - alpha)
    with alpha = plane 3 / 255, BEFORE the truncation; the uint8 image: v clamped to [0, 255] and truncated; the labels cand_labels[index])."""
    wt, canvas = wt.to(dtype), canvas.to(dtype)
    alpha = wt[:, 3:4] / 255
    v = wt[:, :3] * alpha + canvas * (1 - alpha)
    return v, v.clamp(0, 255).to(torch.uint8), cand_labels[torch.as_tensor(index, dtype=torch.long, device=cand_labels.device)]


def aug_inverse(fwd, dtype=torch.float64):
    """The inverse half of frtm_aug_transforms: fwd (n,6) fp32 forward matrices -> (n,6) inverses in `dtype`; the identity where the
    determinant is 0 (a spec of scale 0)."""
    f = fwd.to(dtype)
    a, b, tx, c, d, ty = f.unbind(1)
    det = a * d - b * c
    ok = det != 0
    det = torch.where(ok, det, torch.ones_like(det))
    inv = torch.stack((d / det, -b / det, (b * ty - d * tx) / det, -c / det, a / det, (c * tx - a * ty) / det), 1)
    eye = torch.tensor([1, 0, 0, 0, 1, 0], dtype=dtype, device=f.device).expand_as(inv)
    return torch.where(ok[:, None], inv, eye)


BLEND_SIZES = [(1, 1), (33, 47), (513, 512)]          # 513 x 512 passes the 1024-block cap


def blend_inputs(n, Hh, Ww, alpha):
    """wt (n,4,H,W), canvas (n,3,H,W), cand_labels (n + 2,H,W), index (a permutation offset, with a repeat when n > 1).  alpha: 'zero', 'one'
    (plane 3 exactly 0 / 255) or 'random'.  Colours run from -20 to 280 and the first pixels hold 12.99, 13.0 and 254.999 in target and canvas."""
    g = gen(n, Hh, Ww, 11)
    wt = torch.rand(n, 4, Hh, Ww, generator=g) * 300 - 20
    canvas = torch.rand(n, 3, Hh, Ww, generator=g) * 300 - 20
    special = torch.tensor([12.99, 13.0, 254.999, -0.5, 255.5, 0.999])[:Hh * Ww]
    wt[:, :3].reshape(n, 3, -1)[:, :, :special.numel()] = special
    canvas.reshape(n, 3, -1)[:, :, :special.numel()] = special.flip(0) if Hh * Ww > 1 else special
    wt[:, 3] = {'zero': torch.zeros(n, Hh, Ww), 'one': torch.full((n, Hh, Ww), 255.0), 'random': torch.rand(n, Hh, Ww, generator=g) * 255}[alpha]
    labels = torch.randint(0, 2, (n + 2, Hh, Ww), generator=g).to(torch.uint8)
    index = [(n + 1 - j) for j in range(n)]
    if n > 1:
        index[-1] = index[0]
    return wt, canvas, labels, index
