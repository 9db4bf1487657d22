"""Float64 definition, error bounds and case table of grouped target-model scoring (csrc/target_apply_grouped.hip), written from the contract
in include/frtm_hip.h with no project code.  tests/test_grouped_refs.py pins them on the CPU; tests/test_grouped_scoring_gpu.py and
tests/test_stream_pool_gpu.py hold the kernels to them.

Definition, for one (frame, target) pair: X (Cin, h, w) the frame's features, w1T (Cin, c) the projection in GEMM layout, w2 (1, c, 3, 3):

    cft = w1T^T X          (a 1x1 convolution)              scores = conv2d(cft, w2, padding=1)

Bounds.  Every projected feature is one chain of Cin fused multiply-adds and every score a sum of 9c products: a sum of n terms, each rounded
once per operation in any order, is off by at most gamma(n) * sum |a_i b_i| with gamma(n) = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1).  Hence

    |cft - cft64| <= gamma(Cin + 1) * (|W|^T |X|)
    |s - s64|     <= gamma(9c + 1) * (|f| conv |cft|)  +  |f| conv (gamma(Cin + 1) * |W|^T |X|)

the second line being the rounding of the 3x3 pass over the features the kernel really read plus the projection's own error carried through
the filter.

Case table: small shapes that between them run every compiled form of k_grouped_project<FM, FN> (FM = ceil(c / 32), FN = 2 from
ceil(hw / 64) * G >= 256 on), its row and column tails, one, two and an odd number of K chunks, the empty and ragged channel groups of
k_grouped_scores (16 groups: c = 1, 15, 16, 17), maps one pixel high, one pixel wide and narrower than a 16-pixel tile, a frame pitch that is
no multiple of 4 floats and addresses that are 4-byte but not 16-byte aligned.
"""
import types

import torch
import torch.nn.functional as F

U = 2.0 ** -24
MIXUP_FACTOR = 100.0      # a mixed-up pair, frame or layout must miss the bound by this factor somewhere (tests/test_grouped_refs.py)


def gamma(n):
    return n * U / (1 - n * U)


def reference(Cin, c, X, w1T, w2):
    """Float64 results of ONE pair and what does not depend on the kernel's output: -> (cft64 (1,c,h,w), b1 (1,c,h,w), s64 (1,1,h,w),
    carried (1,1,h,w) = the projection's bound taken through |w2|).  X (Cin,h,w), w1T (Cin,c), w2 (1,c,3,3)."""
    h, w = X.shape[-2:]
    X64, W64, f64 = X.double().reshape(Cin, h * w), w1T.double(), w2.double()
    cft64 = (W64.t() @ X64).reshape(1, c, h, w)
    b1 = gamma(Cin + 1) * (W64.abs().t() @ X64.abs()).reshape(1, c, h, w)
    return cft64, b1, F.conv2d(cft64, f64, padding=1), F.conv2d(b1, f64.abs(), padding=1)


def _bounds(Cin, c, X, w1T, w2, cft):
    """fp64 results and the two bounds of the module docstring for ONE pair: X (Cin,h,w), w1T (Cin,c), w2 (1,c,3,3), cft the kernel's -- of this
    pair, or (n,c,h,w) of n launches of it: b2 is then (n,1,h,w), one bound per launch."""
    h, w = X.shape[-2:]
    cft64, b1, s64, carried = reference(Cin, c, X, w1T, w2)
    b2 = gamma(9 * c + 1) * F.conv2d(cft.double().abs().reshape(-1, c, h, w), w2.double().abs(), padding=1) + carried
    return cft64, b1, s64, b2


def _worst(got, ref, bound):
    err = (got.double().reshape(ref.shape) - ref).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp(min=1e-300)).max())


# ---------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------
WEIGHT_SETS = 5           # pair p uses weight set p % min(G, 5): with frames cycling over 3, neighbouring pairs share neither


def _cycle(G, frames=3):
    return [p % frames for p in range(G)]


# name: (Cin, c, h, w, frames, frame_of_pair, extra floats between frames, feats / w1T[1 % sets] / w2[2 % sets] start one float into their storage)
CASES = {
    # FN = 1 (32-pixel tiles): every c of the row tails, every hw of the column tails
    'c1-1x1': (32, 1, 1, 1, 1, [0], 0, False),                      # one chunk, one pixel, one channel: 15 of 16 channel groups empty
    'c8-1x15': (64, 8, 1, 15, 2, [1, 0, 1], 3, True),               # two chunks: each LDS buffer used once; h = 1; pitch = 3 mod 4
    'c15-4x4': (32, 15, 4, 4, 2, [0, 1], 0, False),                 # last channel group empty
    'c16-17x1': (96, 16, 17, 1, 3, [2, 0, 1, 1], 0, False),         # three chunks; w = 1 with h > 1; two pixel tiles of the scores, one lane live
    'c17-1x31': (32, 17, 1, 31, 2, [0, 1, 0], 5, False),            # ragged groups: 8 of two channels, 1 of one, 7 empty
    'c31-4x8': (160, 31, 4, 8, 2, [1, 1, 0], 0, True),              # five chunks; 32 pixels: the column tile exactly
    'c32-3x11': (64, 32, 3, 11, 3, [0, 1, 2], 0, False),            # BM = c = 32; 33 pixels: one column past the first tile
    'c33-9x7': (96, 33, 9, 7, 2, [0, 1, 1], 1, False),              # one row into FM = 2; w = 7: a 16-pixel tile on three rows
    'c63-8x8': (32, 63, 8, 8, 3, [0, 0, 1, 2, 2], 0, False),        # 5 pairs on 3 frames (the skip test's launch)
    'c65-13x5': (64, 65, 13, 5, 2, [1, 0], 7, True),                # one row into FM = 3; w = 5: a 16-pixel tile on four rows; 65 pixels
    'c96-3x5': (160, 96, 3, 5, 2, [0, 1, 0], 0, False),             # the product's c on a map below one tile of either kernel
    'c97-4x4': (96, 97, 4, 4, 2, [1, 0], 2, False),                 # one row into FM = 4
    'c127-17x1': (64, 127, 17, 1, 3, [2, 1, 0], 0, True),
    'c128-9x7': (32, 128, 9, 7, 2, [0, 1], 0, False),               # every row of the largest tile; 8 channels per group
    # FN = 2 (64-pixel tiles), one per FM: 256 pairs on a map of at most 64 pixels, or 128 on 65 .. 128
    'fn2-c8-8x8': (32, 8, 8, 8, 3, _cycle(256), 0, False),          # 64 pixels: the pairs (255, 256) sit on either side of the switch
    'fn2-c33-13x5': (64, 33, 13, 5, 3, _cycle(128), 2, True),       # 65 pixels: the second tile holds one column
    'fn2-c96-3x5': (32, 96, 3, 5, 3, _cycle(256), 0, False),
    'fn2-c127-1x15': (64, 127, 1, 15, 3, _cycle(256), 1, False),
}
FN1_PER_FM = {1: 'c8-1x15', 2: 'c33-9x7', 3: 'c96-3x5', 4: 'c127-17x1'}
FN2_PER_FM = {1: 'fn2-c8-8x8', 2: 'fn2-c33-13x5', 3: 'fn2-c96-3x5', 4: 'fn2-c127-1x15'}
SWITCH = ('fn2-c8-8x8', 255, 256)
SKIP = 'c63-8x8'


def make(name, draw=0):
    """The case's data, fp32 values from a seeded CPU generator: store (frames * pitch), X (frames, Cin, h, w) a view of it, w1T / w2 the weight
    sets, fop / wop the frame and the weight set of every pair.  ``draw`` = 1: a second, independent draw of the same shapes."""
    Cin, c, h, w, frames, fop, extra, offset = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 7919 * draw)
    pitch = Cin * h * w + extra
    store = torch.randn(frames, pitch, generator=g).relu()                                   # ReLU'd normal features
    sets = min(len(fop), WEIGHT_SETS)
    w1T = [torch.randn(Cin, c, generator=g) / Cin ** 0.5 for _ in range(sets)]               # GEMM layout [Cin][c]
    w2 = [torch.randn(1, c, 3, 3, generator=g) / (9 * c) ** 0.5 for _ in range(sets)]
    return types.SimpleNamespace(name=name, Cin=Cin, c=c, h=h, w=w, frames=frames, fop=list(fop), wop=[p % sets for p in range(len(fop))],
                                 sets=sets, pitch=pitch, offset=bool(offset), store=store, w1T=w1T, w2=w2,
                                 X=store[:, :Cin * h * w].reshape(frames, Cin, h, w))


def combos(case):
    """{(frame, weight set): [pairs]} of a case, in pair order."""
    out = {}
    for p, key in enumerate(zip(case.fop, case.wop)):
        out.setdefault(key, []).append(p)
    return out
