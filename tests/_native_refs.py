"""The definition of csrc/native_size.hip's operator on the CPU, in fp64 from the fp32 taps, and the inputs its tests share.

    m_k   = bilinear sample of plane k (ATen's upsample_bilinear2d, align_corners=False: the taps of csrc/resample_taps.h, which are
            fp32 quantities; the sum over them is taken in fp64 here), the plane itself when the sizes agree
    arg   = first k with the largest m_k;   label = arg if arg >= 1 and m_arg > 0.5 else 0
    margin = min(top - second, |top - 0.5|): how far a pixel is from changing its label

The kernel's fp32 sum is at most six roundings away from the fp64 one on values in [0, 1] (two products and a sum per row pair, two
products and a sum across): SOFT_TOL = 2^-21 covers them (6 * 2^-24 < 2^-21), and a label may differ only where the margin is within
LABEL_MARGIN = 2^-20, twice that."""
import numpy as np
import torch

SOFT_TOL = 2.0 ** -21
LABEL_MARGIN = 2.0 ** -20
EXCLUDED_CAP = 0.01

# (planes, working (h, w), native (H, W))
SHAPES = [
    (2, (5, 7), (9, 13)),
    (3, (13, 9), (5, 3)),            # native smaller than working
    (2, (1, 1), (4, 4)),
    (4, (6, 10), (6, 10)),           # identity
    (3, (17, 70), (40, 300)),        # several tiles per row (it enlarges: every tile's footprint is one staged chunk)
    (16, (9, 11), (23, 31)),
    # (the first six: the shapes the option was specified with; the band the GPU tests exclude holds none of their pixels)
    # native under half the working size: a tile's source footprint exceeds one staged chunk of 36 rows x 132 columns
    (3, (100, 300), (20, 70)),       # 3 row chunks x 3 column chunks per tile, two tiles per row and per column
    (3, (40, 400), (40, 64)),        # rows at equal size (one row chunk of 17 rows), the 400 columns of the one tile column in 4 chunks
]


def merged(planes, h, w, seed):
    """Merged masks (planes, h, w) fp32 made the way k_track_merge makes them: smooth random logits, sigmoid, clamp, merge (background =
    min(1 - p), soft-max of the odds, the winner keeps its probability and every other plane is 0)."""
    n = planes - 1
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(n, max(1, h // 4 + 1), max(1, w // 4 + 1), generator=g, dtype=torch.float64) * 4
    lo = torch.nn.functional.interpolate(lo[None], (h, w), mode='bilinear', align_corners=False)[0] if (h > 1 or w > 1) else lo[:, :1, :1]
    lo = (lo + 0.3 * torch.randn(n, h, w, generator=g, dtype=torch.float64)).float()
    p = torch.sigmoid(lo).clamp(1e-7, 1 - 1e-7)
    bg = (1 - p).min(0, keepdim=True)[0]
    p = torch.cat([bg, p])
    pr = torch.softmax(p / (1 - p), 0)
    arg, win = pr.argmax(0), pr.max(0)[0]
    m = torch.zeros_like(pr)
    m.scatter_(0, arg[None], win[None])
    return m.float().contiguous()


def taps(n_in, n_out):
    """bilinear_taps of csrc/resample_taps.h for every output index as the device code computes them -> (i0, i1, l0, l1), fp32 each.
    The scale is one fp32 division; the source coordinate scale * (d + .5) - .5 is ONE fused multiply-add on the device (HIP's
    __fmul_rn / __fsub_rn are the plain operators, which hipcc contracts, as it does in ATen's own kernel), so it is rounded once: here
    the product of two fp32 numbers and the difference are exact in fp64 and rounded to fp32 at the end."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    d = np.arange(n_out, dtype=np.float64)
    src = (np.float64(scale) * (d + 0.5) - 0.5).astype(np.float32)
    src = np.where(src < 0, f(0), src).astype(np.float32)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (f(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def native_planes(m, size):
    """The fp64 definition: m (K, h, w) fp32 -> (K, H, W) fp64."""
    K, h, w = m.shape
    H, W = size
    m64 = m.double().numpy()
    if (h, w) == (H, W):
        return torch.from_numpy(m64.copy())
    y0, y1, ly0, ly1 = taps(h, H)
    x0, x1, lx0, lx1 = taps(w, W)
    ly0, ly1 = ly0.astype(np.float64)[None, :, None], ly1.astype(np.float64)[None, :, None]
    lx0, lx1 = lx0.astype(np.float64)[None, None, :], lx1.astype(np.float64)[None, None, :]
    top = lx0 * m64[:, y0][:, :, x0] + lx1 * m64[:, y0][:, :, x1]
    bot = lx0 * m64[:, y1][:, :, x0] + lx1 * m64[:, y1][:, :, x1]
    return torch.from_numpy(ly0 * top + ly1 * bot)


def decode(planes):
    """(K, H, W) -> (plane index of the label (H, W) int64, margin (H, W))."""
    top = planes.max(0)[0]
    K = planes.shape[0]
    idx = torch.arange(K).view(K, 1, 1).expand_as(planes)
    arg = torch.where(planes == top[None], idx, torch.full_like(idx, K)).min(0)[0]      # the FIRST index of the maximum
    label = torch.where((arg >= 1) & (top > 0.5), arg, torch.zeros_like(arg))
    if planes.shape[0] > 1:
        second = planes.sort(0, descending=True)[0][1]
        margin = torch.minimum(top - second, (top - 0.5).abs())
    else:
        margin = (top - 0.5).abs()
    return label, margin


def nearest_index(src, dst):
    """F.interpolate(mode='nearest')'s source index: min(floor(d * (float32(src) / dst)), src - 1), the product in float32."""
    s = np.float32(src) / np.float32(dst)
    return np.minimum(np.floor((np.arange(dst, dtype=np.float32) * s).astype(np.float32)).astype(np.int64), src - 1)
