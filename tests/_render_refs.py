"""The renderer of csrc/frame_render.hip stated in numpy: every output byte is an integer function of the inputs (include/frtm_hip.h), so
the GPU tests (tests/test_frame_render_gpu.py) compare byte for byte; tests/test_frame_render.py checks the statement itself (mix against
exact rational rounding, the forward colour table against the fp64 matrices).  Works in the replicated 4:4:4 domain -- every pixel's three
channel bytes -- and box-subsamples the chroma of an NV12 result.

    mix(s, c, a) = (t + (t >> 8)) >> 8,  t = s (255 - a) + c a + 128
    hard: out = mix(s, c_id, a_id); with edge_alpha an object's pixel with a 4-neighbour of another label inside the picture takes edge_alpha
    soft: m = clamp(m_k*, 0, 1), k* the first k >= 1 with the largest m_k; out = rint(float32(m (F - B) + B)), B / F = mix with lut[0] / lut[k*]
    NV12: U', V' = (sum over the block's cnt picture pixels + cnt // 2) // cnt"""
import numpy as np

import _decoder_refs as D

# the issue's forward table: name -> (y0, yr, yg, yb, ur, ug, ub, vr, vg, vb)
FORWARD = {
    'nv12_bt601': (16, 16829, 33039, 6416, -9714, -19071, 28784, 28784, -24103, -4681),
    'nv12_bt601_full': (0, 19595, 38470, 7471, -11058, -21710, 32768, 32768, -27439, -5329),
    'nv12_bt709': (16, 11966, 40254, 4064, -6596, -22189, 28784, 28784, -26145, -2639),
    'nv12_bt709_full': (0, 13933, 46871, 4732, -7509, -25259, 32768, 32768, -29763, -3005),
}


def mix(s, c, a):
    s, c, a = (np.asarray(v).astype(np.int64) for v in (s, c, a))
    t = s * (255 - a) + c * a + 128
    return (t + (t >> 8)) >> 8


def real_forward(name):
    """(y0, 3 x 3 matrix) of the standard's forward transform as real numbers (limited range: luma scaled by 219/255, chroma by 224/255)."""
    kr, kb = D.LUMA[name.split('_')[1]]
    kg = 1.0 - kr - kb
    full = name.endswith('_full')
    ys, cs = (1.0, 1.0) if full else (219.0 / 255.0, 224.0 / 255.0)
    m = np.array([[kr * ys, kg * ys, kb * ys],
                  [-kr / (2 * (1 - kb)) * cs, -kg / (2 * (1 - kb)) * cs, 0.5 * cs],
                  [0.5 * cs, -kg / (2 * (1 - kr)) * cs, -kb / (2 * (1 - kr)) * cs]])
    return (0 if full else 16), m


def rgb_to_yuv(rgb, name):
    """(..., 3) RGB -> (..., 3) uint8 (Y, U, V) by the fixed-point forward formula."""
    y0, yr, yg, yb, ur, ug, ub, vr, vg, vb = FORWARD[name]
    c = np.asarray(rgb).astype(np.int64)
    r, g, b = c[..., 0], c[..., 1], c[..., 2]
    yuv = np.stack([y0 + ((yr * r + yg * g + yb * b + 32768) >> 16), 128 + ((ur * r + ug * g + ub * b + 32768) >> 16),
                    128 + ((vr * r + vg * g + vb * b + 32768) >> 16)], axis=-1)
    return np.clip(yuv, 0, 255).astype(np.uint8)


def rgb_to_yuv_real(rgb, name):
    y0, m = real_forward(name)
    v = np.asarray(rgb).astype(np.float64) @ m.T + np.array([y0, 128.0, 128.0])
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def style_table(palette, alpha=128, background=None, name=None):
    """RenderStyle's (256, 4) table restated: palette and alpha, row 0 = the background (a_0 = 0 when None); ``name``: an NV12 format whose
    (Y, U, V) the colours are given in."""
    t = np.zeros((256, 4), dtype=np.uint8)
    t[:, :3] = palette
    t[:, 3] = alpha
    if background is None:
        t[0, 3] = 0
    else:
        t[0] = background
    if name is not None:
        t[:, :3] = rgb_to_yuv(t[:, :3], name)
    return t


def decode_labels(stack, lut):
    """frtm_masks_to_native's rule on a (K, h, w) float32 stack: arg = the first k with the largest m_k (a NaN never wins),
    id = lut[arg] if arg >= 1 and m_arg > 0.5f else lut[0]."""
    stack = np.asarray(stack, dtype=np.float32)
    best = np.full(stack.shape[1:], -np.inf, dtype=np.float32)
    arg = np.zeros(stack.shape[1:], dtype=np.int64)
    for k in range(stack.shape[0]):
        with np.errstate(invalid='ignore'):
            up = stack[k] > best
        best, arg = np.where(up, stack[k], best), np.where(up, k, arg)
    with np.errstate(invalid='ignore'):
        plane = np.where((arg >= 1) & (best > np.float32(0.5)), arg, 0)
    return np.asarray(lut, dtype=np.uint8)[plane]


def soft_terms(stack):
    """(m float32 in [0, 1], k*) of the soft rule; no plane above -inf (K = 1, NaNs only): m = 0, k* = 1."""
    stack = np.asarray(stack, dtype=np.float32)
    best = np.full(stack.shape[1:], -np.inf, dtype=np.float32)
    ks = np.ones(stack.shape[1:], dtype=np.int64)
    for k in range(1, stack.shape[0]):
        with np.errstate(invalid='ignore'):
            up = stack[k] > best
        best, ks = np.where(up, stack[k], best), np.where(up, k, ks)
    return np.fmin(np.fmax(best, np.float32(0)), np.float32(1)).astype(np.float32), ks


def edge_mask(labels, bg):
    """True where a pixel of an object (label != bg) has a 4-neighbour inside the picture with another label."""
    p = np.pad(labels, 1, mode='edge')                                  # a neighbour beyond the border is the pixel itself
    c = p[1:-1, 1:-1]
    diff = (p[:-2, 1:-1] != c) | (p[2:, 1:-1] != c) | (p[1:-1, :-2] != c) | (p[1:-1, 2:] != c)
    return diff & (c != bg)


def render_444(s, answer, lut, table, soft=False, edge_alpha=None):
    """s: (3, h, w) channel bytes; answer: (h, w) uint8 labels or (K, h, w) float32 stack with its ``lut``; table: (256, 4) -> (3, h, w) uint8."""
    s = np.asarray(s).astype(np.int64)
    table = np.asarray(table).astype(np.int64)
    answer = np.asarray(answer)
    stack = answer.ndim == 3
    if soft:
        assert stack and edge_alpha is None
        m, ks = soft_terms(answer)
        lut = np.asarray(lut, dtype=np.uint8)
        b = table[int(lut[0])]
        f = table[lut[ks]] if answer.shape[0] > 1 else np.broadcast_to(b, ks.shape + (4,))
        out = np.empty_like(s)
        for c in range(3):
            B, F = mix(s[c], b[c], b[3]), mix(s[c], f[..., c], f[..., 3])
            v = (m.astype(np.float64) * (F - B).astype(np.float64) + B.astype(np.float64)).astype(np.float32)    # one rounding, like fmaf
            out[c] = np.rint(v).astype(np.int64)
        return out.astype(np.uint8)
    labels = decode_labels(answer, lut) if stack else answer.astype(np.uint8)
    st = table[labels]
    a = st[..., 3]
    if edge_alpha is not None:
        a = np.where(edge_mask(labels, int(lut[0]) if stack else 0), int(edge_alpha), a)
    return np.stack([mix(s[c], st[..., c], a) for c in range(3)]).astype(np.uint8)


def nv12_444(buf, h, w, pitch, uv_off):
    """The (3, h, w) replicated Y, U, V of a surface: picture samples only."""
    buf = np.asarray(buf)
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    ui = uv_off + (y >> 1) * pitch + 2 * (x >> 1)
    return np.stack([buf[y * pitch + x], buf[ui], buf[ui + 1]])


def store_nv12(dst, yuv, pitch, uv_off):
    """The (3, h, w) per-pixel results into a COPY of surface ``dst``: Y per pixel, chroma box-subsampled; only picture samples change."""
    out = np.array(dst, dtype=np.uint8, copy=True)
    _, h, w = yuv.shape
    for y in range(h):
        out[y * pitch:y * pitch + w] = yuv[0, y]
    for j in range((h + 1) // 2):
        for i in range((w + 1) // 2):
            for c in (1, 2):
                blk = yuv[c, 2 * j:min(2 * j + 2, h), 2 * i:min(2 * i + 2, w)].astype(np.int64)
                out[uv_off + j * pitch + 2 * i + c - 1] = (int(blk.sum()) + blk.size // 2) // blk.size
    return out


def render_nv12(src, h, w, pitch, uv_off, dst, dpitch, duv, answer, lut, table, soft=False, edge_alpha=None):
    return store_nv12(dst, render_444(nv12_444(src, h, w, pitch, uv_off), answer, lut, table, soft, edge_alpha), dpitch, duv)


def merged_stack(rng, K, h, w):
    """A merged-like (K, h, w) float32 stack: one plane nonzero per pixel, its value uniform in (0, 1); blobs of a few pixels so that
    objects have boundaries."""
    bh, bw = max(1, h // 5), max(1, w // 7)
    owner = rng.integers(0, K, ((h + bh - 1) // bh, (w + bw - 1) // bw))
    owner = np.kron(owner, np.ones((bh, bw), dtype=np.int64))[:h, :w]
    val = rng.uniform(0.05, 1.0, (h, w)).astype(np.float32)
    return np.where(owner[None] == np.arange(K)[:, None, None], val[None], np.float32(0)).astype(np.float32)


def hand_placed(stack):
    """The pixels the decode and the soft clamp can get wrong, written over the first pixels of the picture (as many as it has)."""
    K, h, w = stack.shape
    if K < 2:
        return stack
    cases = [{1: 0.5}, {1: 1.5}, {1: -0.25}, {1: np.nan}]               # 0.5 decodes to the background; the clamp; a NaN gives m = 0
    if K > 2:
        cases += [{1: 0.75, 2: 0.75}, {1: np.nan, 2: 0.625}, {0: 0.9, 1: 0.75, 2: 0.8}]     # the first of two equal planes wins
    flat = stack.reshape(K, -1)
    for i, case in enumerate(cases[:h * w]):
        flat[:, i] = 0
        for k, v in case.items():
            flat[k, i] = v
    return stack


def blob_labels(rng, h, w, ids):
    bh, bw = max(1, h // 4), max(1, w // 6)
    owner = rng.integers(0, len(ids), ((h + bh - 1) // bh, (w + bw - 1) // bw))
    return np.asarray(ids, dtype=np.uint8)[np.kron(owner, np.ones((bh, bw), dtype=np.int64))[:h, :w]]
