"""fp64 restatements of the three operators of csrc/frame_resize.hip (frtm_resize_frames_u8 modes area and cubic, frtm_resize_labels_u8),
as dense per-axis weight matrices: out = My @ plane @ Mx^T.  Shared by tests/test_frame_resize.py (which checks the restatements against
torch where torch has the operator) and tests/test_frame_resize_gpu.py (which checks the kernels against them).

Tap positions and phases are formed from Python integers, so the only rounding in a weight is its final float64 division."""
import numpy as np

NEAR_TIE = 1e-3          # |frac(fp64 value) - 0.5| within which an fp32 sum may round the other way (tests/test_frame_resize_gpu.py)


def _phase(src, dst):
    """Half-pixel source coordinate (d + 0.5) src / dst - 0.5 of every output index as (floor, fraction)."""
    d = np.arange(dst, dtype=np.int64)
    num, den = (2 * d + 1) * src - dst, 2 * dst
    fl = num // den                                      # floors towards -inf
    return fl, (num - fl * den) / den


def area_matrix(src, dst):
    """(dst, src) float64.  src >= dst: the share of source pixel s in the interval [d src/dst, (d + 1) src/dst), normalised to 1 (the
    identity for src == dst); src < dst: bilinear with half-pixel centres and a replicate border."""
    m = np.zeros((dst, src))
    if src >= dst:
        s, d = np.arange(src, dtype=np.int64)[None], np.arange(dst, dtype=np.int64)[:, None]
        overlap = np.minimum((s + 1) * dst, (d + 1) * src) - np.maximum(s * dst, d * src)      # in units of 1 / dst pixel
        return np.clip(overlap, 0, None) / src
    fl, t = _phase(src, dst)
    for k, wgt in ((0, 1 - t), (1, t)):
        np.add.at(m, (np.arange(dst), np.clip(fl + k, 0, src - 1)), wgt)
    return m


def _cubic(x, a=-0.75):
    x = np.abs(x)
    return np.where(x <= 1, ((a + 2) * x - (a + 3)) * x * x + 1, ((a * x - 5 * a) * x + 8 * a) * x - 4 * a)


def cubic_matrix(src, dst):
    """(dst, src) float64: cubic convolution (a = -0.75) at the half-pixel source coordinate (not clamped at 0), the four taps' indices
    clamped into the map -- F.interpolate(mode='bicubic', align_corners=False) for a given output size."""
    m = np.zeros((dst, src))
    fl, t = _phase(src, dst)
    for k in (-1, 0, 1, 2):
        np.add.at(m, (np.arange(dst), np.clip(fl + k, 0, src - 1)), _cubic(t - k))
    return m


def resize_ref(planes_u8, size, mode):
    """planes_u8: (P, h, w) uint8 array -> (P, H, W) float64, not rounded.  mode: 'area' or 'cubic'."""
    matrix = {'area': area_matrix, 'cubic': cubic_matrix}[mode]
    x = np.asarray(planes_u8, dtype=np.float64)
    my, mx = matrix(x.shape[1], size[0]), matrix(x.shape[2], size[1])
    return my @ x @ mx.T


def round_u8(v):
    """Nearest, ties to even, clamped to 0..255."""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def near_tie(v):
    """Where the fp64 value sits within NEAR_TIE of a rounding boundary."""
    return np.abs(v - np.floor(v) - 0.5) <= NEAR_TIE


def nearest_index(src, dst):
    """Source index of every output index under F.interpolate(mode='nearest'): min(floor(d * (float32(src) / float32(dst))), src - 1),
    the product in float32."""
    scale = np.float32(src) / np.float32(dst)
    return np.minimum(np.floor(np.arange(dst, dtype=np.float32) * scale).astype(np.int64), src - 1)


def label_ref(label_u8, obj_id, size):
    """label_u8: (h, w) uint8 -> (H, W) uint8 = (label == obj_id) sampled at the nearest-neighbour indices."""
    lb = np.asarray(label_u8)
    ys, xs = nearest_index(lb.shape[0], size[0]), nearest_index(lb.shape[1], size[1])
    return (lb[ys][:, xs] == obj_id).astype(np.uint8)


def assert_band(got_u8, ref64, what):
    """The criterion of the resize tests: equal to the half-even rounding of the fp64 value wherever that value is farther than NEAR_TIE
    from a tie, at most 1 LSB off elsewhere.  Returns (mismatches inside the band, share of outputs inside the band)."""
    got, want, band = np.asarray(got_u8).astype(np.int64), round_u8(ref64).astype(np.int64), near_tie(ref64)
    diff = np.abs(got - want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert int((diff[~band] != 0).sum()) == 0, '%s: %d outputs differ outside the near-tie band (max %d)' % (what, int((diff[~band] != 0).sum()), int(diff.max()))
    assert int(diff.max()) <= 1, '%s: off by %d inside the near-tie band' % (what, int(diff.max()))
    return int((diff != 0).sum()), float(band.mean())


# The mixed call of tests/test_frame_resize_gpu.py: (h, w, mode) of seven frames resized to TARGET in ONE launch, packed back to back
# (3 * 45 * 77 is odd: most bases are misaligned).  Ratios per axis: 1.5 / 1.51; one axis only (83 / 51; 68 / 51 = 4 / 3 would put a third
# of the outputs ON a tie, which says nothing about the kernel: that shape is checked for exact equality in the extra cases instead);
# the identity; 7.3 / 3.1 (a footprint of several LDS chunks of rows); exactly 2; one axis reduced and one enlarged; cubic enlarging.
TARGET = (30, 51)
MIXED = [(45, 77, 'area'), (30, 83, 'area'), (30, 51, 'area'), (219, 160, 'area'), (60, 102, 'area'), (33, 40, 'area'), (20, 30, 'cubic')]
IDENTITY, RATIO2, CUBIC = 2, 4, 6
# Further frames, a second launch: footprints of several chunks of COLUMNS in both modes (520 / 51 = 10.2), cubic reducing, a one-pixel-wide
# and a one-pixel-high source, and the 4 / 3 frame, whose weights (3/4, 1/4, 1/2) and sums are exact in fp32.
EXTRA = [(37, 520, 'area'), (37, 520, 'cubic'), (95, 130, 'cubic'), (300, 1, 'area'), (1, 7, 'cubic'), (30, 68, 'area')]
EXACT_EXTRA = 5
BAND_CAP = 0.01          # share of outputs a non-integer-ratio frame may have inside the near-tie band (uniform fractions: 0.2 %)


def seeded_frames(shapes, seed, planes=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (planes, h, w), dtype=np.uint8) for h, w, _ in shapes]
CAPPED_MIXED, CAPPED_EXTRA = [0, 1, 3, 5, 6], [0, 1, 2]          # the frames of non-integer ratio: the cap applies to them
