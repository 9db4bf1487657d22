"""Tiny DAVIS- and YouTube-VOS-shaped trees on disk (JPEG frames, palette PNG annotations) for the training sample-set tests, and the
occlusion tables they must produce, computed by hand from the rectangle areas below.

Sequence A (6 frames): object 1 covers 400 px except 90 in frame 2 and 120 in frame 4; object 3 covers 600 px except 140 in frame 1;
id 2 never occurs.  Sequence B (5 frames): object 1 covers 300 px throughout.  Sequence C (3 frames) is shorter than min_seq_length.
  hard minimum (100 px):              A/1 is occluded in frame 2 (90 px) and nowhere else
  DAVIS fraction rule (0.25 of peak): 90 / 400 and 140 / 600 = 0.233 fall below it, 120 / 400 = 0.3 does not: A/3 is occluded in frame 1
  the background never falls below 1400 of its peak 1860 px."""
import numpy as np

A_AREAS = {1: [400, 400, 90, 400, 120, 400], 3: [600, 140, 600, 600, 600, 600]}
B_AREAS = {1: [300] * 5}
C_AREAS = {1: [300] * 3}


def _occ(n, m, true_at):
    occ = np.zeros((n, m), dtype=bool)
    for f, o in true_at:
        occ[f, o] = True
    return occ


ABSENT = [(f, 2) for f in range(6)]
DAVIS_OCC_A = _occ(6, 4, ABSENT + [(2, 1), (1, 3)])
YTVOS_OCC_A = _occ(6, 4, ABSENT + [(2, 1)])
OCC_B = _occ(5, 2, [])


def _write_sequence(jpeg_dir, anno_dir, size, areas, rng, first_stem=0, stem_step=1):
    from PIL import Image
    h, w = size
    jpeg_dir.mkdir(parents=True)
    anno_dir.mkdir(parents=True)
    n = len(next(iter(areas.values())))
    palette = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, 1)
    for f in range(n):
        stem = '%05d' % (first_stem + f * stem_step)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(jpeg_dir / (stem + '.jpg'), quality=90)
        lb = np.zeros((h, w), dtype=np.uint8)
        for band, (obj, a) in enumerate(sorted(areas.items())):       # object k lives in its own band of h // 2 rows, 10 px per row
            assert a[f] % 10 == 0 and a[f] // 10 <= w and band < 2
            rows, top = 10, band * (h // 2)
            lb[top:top + rows, :a[f] // 10] = obj
        assert all(int((lb == obj).sum()) == a[f] for obj, a in areas.items())
        im = Image.fromarray(lb, 'P')
        im.putpalette(palette.ravel())
        im.save(anno_dir / (stem + '.png'))


def make_davis(root, seed=0):
    """-> root of a DAVIS 2017 tree with the sequences 'alpha' (A, 40 x 60), 'beta' (B, 44 x 64) and 'gamma' (C)."""
    rng = np.random.default_rng(seed)
    for name, size, areas in (('alpha', (40, 60), A_AREAS), ('beta', (44, 64), B_AREAS), ('gamma', (40, 60), C_AREAS)):
        _write_sequence(root / 'JPEGImages' / '480p' / name, root / 'Annotations' / '480p' / name, size, areas, rng)
    (root / 'ImageSets' / '2017').mkdir(parents=True)
    (root / 'ImageSets' / '2017' / 'train.txt').write_text('alpha\nbeta\ngamma\n')
    return root


YTVOS_SIZES = {'0a1b2c': (40, 60), '3d4e5f': (48, 36), '6a7b8c': (40, 60)}


def make_ytvos(root, seed=1):
    """-> root of a YouTube-VOS tree: '0a1b2c' (A, landscape 40 x 60), '3d4e5f' (B, portrait 48 x 36), '6a7b8c' (C); frames every 5."""
    rng = np.random.default_rng(seed)
    for name, areas in (('0a1b2c', A_AREAS), ('3d4e5f', B_AREAS), ('6a7b8c', C_AREAS)):
        _write_sequence(root / 'train' / 'JPEGImages' / name, root / 'train' / 'Annotations' / name, YTVOS_SIZES[name], areas, rng, stem_step=5)
    return root
