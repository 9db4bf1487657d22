"""The colour conversion of csrc/frame_formats.hip stated in numpy, and an encoder that makes NV12 buffers for the tests.  Shared by
tests/test_decoder_frames.py (the formula against the fp64 matrices) and tests/test_decoder_frames_gpu.py (the kernel against the formula).

The formula (include/frtm_hip.h): with yy = Y - y0, u = U - 128, v = V - 128 in int32,
    R = clamp(floor((a yy + rv v + 32768) / 65536), 0, 255)
    G = clamp(floor((a yy - gu u - gv v + 32768) / 65536), 0, 255)
    B = clamp(floor((a yy + bu u + 32768) / 65536), 0, 255)
each coefficient round(65536 * c) of the standard matrices; chroma replicated over its 2 x 2 block."""
import numpy as np

# format name -> (id, y0, a, rv, gu, gv, bu)
FORMATS = {
    'nv12_bt601': (1, 16, 76309, 104597, 25675, 53279, 132201),
    'nv12_bt601_full': (2, 0, 65536, 91881, 22553, 46802, 116130),
    'nv12_bt709': (3, 16, 76309, 117489, 13975, 34925, 138438),
    'nv12_bt709_full': (4, 0, 65536, 103206, 12276, 30679, 121609),
}
NV12 = list(FORMATS)
# (Kr, Kb) of the two standards: the real-valued matrices are derived from these alone
LUMA = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}


def real_coefficients(name):
    """(y0, a, rv, gu, gv, bu) as real numbers: the standard's matrix, limited range scaled by 255/219 (luma) and 255/224 (chroma)."""
    kr, kb = LUMA[name.split('_')[1]]
    kg = 1.0 - kr - kb
    full = name.endswith('_full')
    ys, cs = (1.0, 1.0) if full else (255.0 / 219.0, 255.0 / 224.0)
    return (0 if full else 16, ys, 2 * (1 - kr) * cs, 2 * (1 - kb) * kb / kg * cs, 2 * (1 - kr) * kr / kg * cs, 2 * (1 - kb) * cs)


def yuv_to_rgb(Y, U, V, name):
    """The integer formula on arrays of equal shape -> (R, G, B) uint8."""
    _, y0, a, rv, gu, gv, bu = FORMATS[name]
    yy, u, v = Y.astype(np.int64) - y0, U.astype(np.int64) - 128, V.astype(np.int64) - 128
    assert max(np.abs(a * yy).max() + np.abs(gu * u).max() + np.abs(gv * v).max(), np.abs(bu * u).max() + np.abs(a * yy).max()) < 6e7
    r = (a * yy + rv * v + 32768) >> 16                                # (>> floors, like //)
    g = (a * yy - gu * u - gv * v + 32768) >> 16
    b = (a * yy + bu * u + 32768) >> 16
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in (r, g, b))


def yuv_to_rgb_real(Y, U, V, name):
    """clamp(rint(fp64 matrix)) -> (R, G, B) uint8."""
    y0, a, rv, gu, gv, bu = real_coefficients(name)
    yy, u, v = Y.astype(np.float64) - y0, U.astype(np.float64) - 128, V.astype(np.float64) - 128
    return tuple(np.clip(np.rint(c), 0, 255).astype(np.uint8) for c in (a * yy + rv * v, a * yy - gu * u - gv * v, a * yy + bu * u))


def nv12_to_rgb(buf, off, h, w, pitch, uv_off, name):
    """The planar (3, h, w) uint8 frame of an NV12 surface in the flat uint8 array ``buf``: only picture samples are read."""
    buf = np.asarray(buf)
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    Y = buf[off + y * pitch + x]
    ui = uv_off + (y >> 1) * pitch + 2 * (x >> 1)
    return np.stack(yuv_to_rgb(Y, buf[ui], buf[ui + 1], name))


def surface_bytes(h, w, pitch, coded_h=None):
    coded_h = h if coded_h is None else coded_h
    return pitch * coded_h + pitch * ((h + 1) // 2)


def sample_mask(h, w, pitch, coded_h=None):
    """Boolean array over a surface's bytes: True where a byte is a picture sample (Y of the picture; U,V of its ceil(h/2) x ceil(w/2) blocks)."""
    coded_h = h if coded_h is None else coded_h
    m = np.zeros(surface_bytes(h, w, pitch, coded_h), dtype=bool)
    for y in range(h):
        m[y * pitch:y * pitch + w] = True
    for r in range((h + 1) // 2):
        o = pitch * coded_h + r * pitch
        m[o:o + 2 * ((w + 1) // 2)] = True
    return m


def random_surface(rng, h, w, pitch, coded_h=None, fill=None):
    """A surface of uniformly random Y, U, V over 0..255 (so that the clamps act); the bytes that are no picture sample are ``fill``
    (None: random as well).  -> (flat uint8 array, uv offset)."""
    coded_h = h if coded_h is None else coded_h
    assert pitch >= 2 * ((w + 1) // 2) and coded_h >= h
    n = surface_bytes(h, w, pitch, coded_h)
    buf = rng.integers(0, 256, n, dtype=np.uint8)
    if fill is not None:
        buf[~sample_mask(h, w, pitch, coded_h)] = fill
    return buf, pitch * coded_h


def encode_nv12(rgb, pitch, name, coded_h=None, fill=0):
    """(3, h, w) uint8 RGB -> (flat uint8 NV12 surface, uv offset): the standard's forward matrix in fp64, chroma the mean of its block
    (edge blocks: of the pixels they have), padding bytes ``fill``.  Makes inputs only: nothing is held to it."""
    _, h, w = rgb.shape
    coded_h = h if coded_h is None else coded_h
    kr, kb = LUMA[name.split('_')[1]]
    kg = 1.0 - kr - kb
    full = name.endswith('_full')
    r, g, b = (rgb[i].astype(np.float64) for i in range(3))
    yf = kr * r + kg * g + kb * b
    cb, cr = (b - yf) / (2 * (1 - kb)), (r - yf) / (2 * (1 - kr))
    y0, ys, cs = (0, 1.0, 1.0) if full else (16, 219.0 / 255.0, 224.0 / 255.0)
    Y = np.clip(np.rint(y0 + ys * yf), 0, 255).astype(np.uint8)
    ch, cw = (h + 1) // 2, (w + 1) // 2

    def block_mean(c):
        p = np.full((2 * ch, 2 * cw), np.nan)
        p[:h, :w] = c
        return np.nanmean(p.reshape(ch, 2, cw, 2), axis=(1, 3))
    U = np.clip(np.rint(128 + cs * block_mean(cb)), 0, 255).astype(np.uint8)
    V = np.clip(np.rint(128 + cs * block_mean(cr)), 0, 255).astype(np.uint8)
    buf = np.full(surface_bytes(h, w, pitch, coded_h), fill, dtype=np.uint8)
    uv_off = pitch * coded_h
    for yy in range(h):
        buf[yy * pitch:yy * pitch + w] = Y[yy]
    for rr in range(ch):
        buf[uv_off + rr * pitch:uv_off + rr * pitch + 2 * cw:2] = U[rr]
        buf[uv_off + rr * pitch + 1:uv_off + rr * pitch + 2 * cw:2] = V[rr]
    return buf, uv_off
