"""The contract of csrc/object_parts.hip (include/frtm_hip.h, frtm_clean_frames) stated in numpy: slots, parts, names, the keep rule, the
twelve words per slot, the cleaned map and the component map -- and, beside it, ``parts_loop``, a plain flood fill over pixels that checks the
numpy statement.  Everything is an exact integer function of the inputs, so the tests compare with ``==``.  Self-contained: the slot rule is
restated here, not imported.

    slot:   stack: arg = the first k with the largest m_k (a NaN never wins); arg if arg >= 1 and m_arg > 0.5f, else 0
            label map: the index of the pixel's id in ``ids`` (the first, if listed twice), none when not listed
    part:   a maximal set of pixels of one slot joined by 4- (8-) neighbour steps; its name: the smallest y w + x among its pixels
    rule:   slot s is ruled when ids[s] != fill; a part of a ruled slot is kept iff area >= min_area and (not largest_only or it is the
            slot's largest part, ties to the smaller name); the parts of an unruled slot are all kept
    words:  parts, kept, area, kept_area, largest_area, largest_name, x_min, y_min, x_max, y_max (of the largest part), ruled, id"""
import numpy as np

SLOTS, WORDS = 16, 12
PARTS, KEPT, AREA, KEPT_AREA, LARGEST_AREA, LARGEST_NAME, X_MIN, Y_MIN, X_MAX, Y_MAX, RULED, ID = range(12)


def decode(stack):
    """(K, h, w) float32 -> (h, w) decoded plane."""
    stack = np.asarray(stack, dtype=np.float32)
    best = np.full(stack.shape[1:], -np.inf, dtype=np.float32)
    arg = np.zeros(stack.shape[1:], dtype=np.int64)
    for k in range(stack.shape[0]):
        with np.errstate(invalid='ignore'):
            up = stack[k] > best
        best, arg = np.where(up, stack[k], best), np.where(up, k, arg)
    with np.errstate(invalid='ignore'):
        return np.where((arg >= 1) & (best > np.float32(0.5)), arg, 0)


def slots(answer, ids):
    """(h, w) int64: the slot of every pixel, -1 for none."""
    answer, ids = np.asarray(answer), [int(v) for v in np.asarray(ids).reshape(-1)]
    if answer.ndim == 3:
        assert answer.shape[0] == len(ids)
        return decode(answer)
    slot = np.full(answer.shape, -1, dtype=np.int64)
    for s in reversed(range(len(ids))):
        slot[answer == ids[s]] = s
    return slot


def _pairs(slot, connectivity):
    """The index pairs (a, b), a > b, of neighbouring pixels with the same slot (>= 0)."""
    h, w = slot.shape
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    a, b = [], []
    for dy, dx in steps:
        lo = (slice(0, h - dy), slice(max(0, -dx), w - max(0, dx)))          # the pixel (y, x)
        hi = (slice(dy, h), slice(max(0, dx), w - max(0, -dx)))              # its neighbour (y + dy, x + dx)
        same = (slot[lo] == slot[hi]) & (slot[lo] >= 0)
        a.append(idx[hi][same])
        b.append(idx[lo][same])
    return np.concatenate(a), np.concatenate(b)


def names(slot, connectivity):
    """(h, w) int64: the name of every pixel's part, -1 without a slot.  Minimum hooking on a forest L[p] <= p: every round hooks the root
    of each end of every pair under the smaller of the two roots, then pointer jumping makes every pixel point at its root again; a round
    at least halves the trees of a part, and when no pair joins two trees the root of a part is its smallest pixel."""
    assert connectivity in (4, 8)
    slot = np.asarray(slot)
    h, w = slot.shape
    L = np.arange(h * w, dtype=np.int64)
    a, b = _pairs(slot, connectivity)
    while True:
        la, lb = L[a], L[b]
        differ = la != lb
        if not differ.any():
            break
        a, b, la, lb = a[differ], b[differ], la[differ], lb[differ]
        m = np.minimum(la, lb)
        np.minimum.at(L, la, m)
        np.minimum.at(L, lb, m)
        while True:
            up = L[L]
            if np.array_equal(up, L):
                break
            L = up
    return np.where(slot.reshape(-1) >= 0, L, -1).reshape(h, w)


def parts_loop(slot, connectivity):
    """``names`` as a flood fill over pixels in plain Python: the seeds come in index order, so a seed is its part's name."""
    slot = np.asarray(slot)
    h, w = slot.shape
    out = np.full((h, w), -1, dtype=np.int64)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    for y0 in range(h):
        for x0 in range(w):
            if slot[y0, x0] < 0 or out[y0, x0] >= 0:
                continue
            name = y0 * w + x0
            out[y0, x0] = name
            todo = [(y0, x0)]
            while todo:
                y, x = todo.pop()
                for dy, dx in steps:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < h and 0 <= xx < w and out[yy, xx] < 0 and slot[yy, xx] == slot[y0, x0]:
                        out[yy, xx] = name
                        todo.append((yy, xx))
    return out


def clean(answer, ids, connectivity=8, min_area=1, largest_only=False, fill=0, part_names=None):
    """One frame -> (labels (h, w) uint8, components (h, w) int32, words (16, 12) int64).  ``part_names``: the names, when the caller has
    them (from parts_loop, say); else ``names``."""
    answer = np.asarray(answer)
    idv = [int(v) for v in np.asarray(ids).reshape(-1)]
    slot = slots(answer, idv)
    h, w = slot.shape
    comp = names(slot, connectivity) if part_names is None else np.asarray(part_names)
    flat, sflat = comp.reshape(-1), slot.reshape(-1)
    area_at = np.bincount(flat[flat >= 0], minlength=h * w)              # a part's pixels, at its name
    keep_at = np.zeros(h * w, dtype=bool)
    words = np.zeros((SLOTS, WORDS), dtype=np.int64)
    for s, oid in enumerate(idv):
        roots = np.unique(flat[sflat == s])
        a = area_at[roots]
        ruled = oid != fill
        big = int(roots[np.lexsort((roots, -a))[0]]) if len(roots) else -1      # the largest area, then the smallest name
        keep = ((a >= min_area) & ((roots == big) | (not largest_only))) if ruled else np.ones(len(roots), dtype=bool)
        keep_at[roots[keep]] = True
        ys, xs = np.nonzero(comp == big) if big >= 0 else (np.array([]), np.array([]))
        box = (xs.min(), ys.min(), xs.max(), ys.max()) if big >= 0 else (w, h, -1, -1)
        words[s] = (len(roots), keep.sum(), a.sum(), a[keep].sum(), area_at[big] if big >= 0 else 0, big) + tuple(box) + (int(ruled), oid)
    kept_pixel = keep_at[np.maximum(flat, 0)] & (flat >= 0)
    labels = np.where(kept_pixel, np.asarray(idv, dtype=np.int64)[np.maximum(sflat, 0)], fill)
    if answer.ndim == 2:
        labels = np.where(sflat >= 0, labels, answer.reshape(-1))        # a label-map pixel without a slot keeps its input byte
    return labels.astype(np.uint8).reshape(h, w), comp.astype(np.int32), words


def partition_of(label_image):
    """A canonical form of a labelling for comparing partitions: every pixel's label replaced by the first index that carries it (0 stays
    'no part', as -1)."""
    flat = np.asarray(label_image).reshape(-1)
    first = {}
    out = np.full(flat.size, -1, dtype=np.int64)
    for p, v in enumerate(flat.tolist()):
        if v:
            out[p] = first.setdefault(v, p)
    return out.reshape(np.asarray(label_image).shape)


# ---- the pictures a union-find gets wrong: (h, w) int64 maps of slots 0 .. K - 1 (object slot `o`, a second one `o2`) ----------------------
def picture(what, h, w, o=1, o2=1, tile=(32, 64), rng=None):
    a = np.zeros((h, w), dtype=np.int64)
    yy, xx = np.mgrid[0:h, 0:w]
    if what == 'background':
        pass
    elif what == 'full':
        a[:] = o
    elif what == 'checker':
        a[(yy + xx) % 2 == 1] = o
    elif what == 'diagonal':
        a[np.arange(h), np.arange(h) % w] = o
    elif what == 'spiral':                                              # rings two apart, each cut open and joined to the next: one path
        y0, x0, y1, x1 = 0, 0, h - 1, w - 1
        while y0 <= y1 and x0 <= x1:
            a[y0, x0:x1 + 1] = o
            a[y0:y1 + 1, x1] = o
            a[y1, x0:x1 + 1] = o
            a[y0 + 2:y1 + 1, x0] = o
            if y0 + 2 <= y1 and x0 + 1 <= x1:
                a[y0 + 2, x0 + 1] = o
            if y0 + 1 <= y1 and x0 < x1:
                a[y0 + 1, x0] = 0
            y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
    elif what in ('comb', 'comb_mirrored'):                             # teeth joined along the last row only -- or along the first
        a[:, ::2] = o
        a[h - 1 if what == 'comb' else 0, :] = o
    elif what == 'serpentine':                                          # crosses every vertical seam in every second row, every horizontal one
        a[::2, :] = o
        for y in range(1, h, 2):
            a[y, 0 if (y // 2) % 2 else w - 1] = o
    elif what == 'ring':                                                # a ring of o around a disc of o2, background in between
        d2 = (yy - h // 2) ** 2 + (xx - w // 2) ** 2
        R = max(min(h, w) // 2 - 2, 0)                                   # (the ring stays off the border: the background outside is one part)
        a[(d2 >= (3 * R // 4) ** 2) & (d2 <= R * R)] = o
        a[d2 <= (R // 4) ** 2] = o2
    elif what == 'equal':                                               # two parts of equal area in one slot: the tie goes to the first
        a[:min(h, 3), :min(w, 2)] = o
        a[h - min(h, 3):, w - min(w, 2):] = o
    elif what == 'corners':                                             # the picture's corners, and both sides of a seam corner
        a[0, 0] = a[0, w - 1] = a[h - 1, 0] = a[h - 1, w - 1] = o
        th, tw = tile
        if th < h and tw < w:
            a[th - 1, tw - 1] = a[th, tw] = o
            a[th - 1, tw] = a[th, tw - 1] = o2
    elif what == 'noise':                                               # uniform noise at p = 0.5 in one slot: many parts, long chains
        a[rng.random((h, w)) < 0.5] = o
    else:
        raise ValueError(what)
    return a


PICTURES = ('background', 'full', 'checker', 'diagonal', 'spiral', 'comb', 'comb_mirrored', 'serpentine', 'ring', 'equal', 'corners', 'noise')
