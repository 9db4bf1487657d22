"""The object report of csrc/object_report.hip stated twice: in numpy (``words``) and as a plain loop over pixels (``words_loop``, for tiny
maps: it checks the numpy statement).  Every word is an exact integer function of the inputs (include/frtm_hip.h), so the GPU tests
(tests/test_object_report_gpu.py) compare all n x 16 x 12 words with ``==``.  Self-contained: the decode is restated here.

    slot:   stack: arg = the first k with the largest m_k (a NaN never wins); arg if arg >= 1 and m_arg > 0.5f, else 0
            label map: the index of the pixel's id in ``ids`` (the first, if listed twice), none when not listed
    label:  the decoded plane, or the id of a label map
    words:  area, x_min, y_min, x_max, y_max (empty: w, h, -1, -1), sum_x, sum_y, edge, border, conf, mass, id;  slots >= K: zeros
    q(m) =  rint(float32(255) * clamp(m, 0, 1)), a NaN gives 0"""
import numpy as np

SLOTS, WORDS = 16, 12
AREA, XMIN, YMIN, XMAX, YMAX, SUMX, SUMY, EDGE, BORDER, CONF, MASS, ID = range(12)


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


def q(m):
    m = np.asarray(m, dtype=np.float32)
    return np.rint(np.float32(255) * np.fmin(np.fmax(m, np.float32(0)), np.float32(1))).astype(np.int64)      # fmax / fmin drop a NaN


def edges(label):
    """True where a pixel has a 4-neighbour inside the picture with another label."""
    p = np.pad(label, 1, mode='edge')                                   # a neighbour beyond the border is the pixel itself
    c = p[1:-1, 1:-1]
    return (p[:-2, 1:-1] != c) | (p[2:, 1:-1] != c) | (p[1:-1, :-2] != c) | (p[1:-1, 2:] != c)


def words(answer, ids):
    """One frame: ``answer`` a (h, w) uint8 label map with the ``ids`` to measure, or a (K, h, w) float32 stack with ``ids`` its LUT
    -> (16, 12) int64."""
    answer, ids = np.asarray(answer), np.asarray(ids, dtype=np.uint8)
    K = ids.size
    h, w = answer.shape[-2:]
    stack = answer.ndim == 3
    if stack:
        assert answer.shape[0] == K
        label = slot = decode(answer)
        qs = q(answer)
    else:
        label = answer.astype(np.int64)
        slot = np.full((h, w), -1, dtype=np.int64)
        for s in reversed(range(K)):
            slot[label == int(ids[s])] = s
    edge = edges(label)
    ys, xs = np.mgrid[:h, :w]
    border = (ys == 0) | (ys == h - 1) | (xs == 0) | (xs == w - 1)
    out = np.zeros((SLOTS, WORDS), dtype=np.int64)
    for s in range(K):
        m = slot == s
        area = int(m.sum())
        out[s, AREA] = area
        out[s, XMIN:YMAX + 1] = (xs[m].min(), ys[m].min(), xs[m].max(), ys[m].max()) if area else (w, h, -1, -1)
        out[s, SUMX], out[s, SUMY] = xs[m].sum(), ys[m].sum()
        out[s, EDGE], out[s, BORDER] = (m & edge).sum(), (m & border).sum()
        if stack:
            out[s, CONF], out[s, MASS] = qs[s][m].sum(), qs[s].sum()
        out[s, ID] = int(ids[s])
    return out


def _q1(m):
    m = float(m)
    if m != m:
        return 0
    return int(np.rint(np.float32(255) * np.float32(min(max(m, 0.0), 1.0))))


def words_loop(answer, ids):
    """``words`` as a loop over pixels in plain Python."""
    answer = np.asarray(answer)
    ids = [int(v) for v in np.asarray(ids).reshape(-1)]
    K = len(ids)
    h, w = answer.shape[-2:]
    stack = answer.ndim == 3

    def label_of(y, x):
        if not stack:
            return int(answer[y, x])
        best, arg = float('-inf'), 0
        for k in range(K):
            if float(answer[k, y, x]) > best:
                best, arg = float(answer[k, y, x]), k
        return arg if arg >= 1 and best > 0.5 else 0

    out = [[0] * WORDS for _ in range(SLOTS)]
    for s in range(K):
        out[s][XMIN], out[s][YMIN], out[s][XMAX], out[s][YMAX], out[s][ID] = w, h, -1, -1, ids[s]
    for y in range(h):
        for x in range(w):
            lab = label_of(y, x)
            if stack:
                for k in range(K):
                    out[k][MASS] += _q1(answer[k, y, x])
                s = lab
            else:
                s = ids.index(lab) if lab in ids else None
            if s is None:
                continue
            o = out[s]
            o[AREA] += 1
            o[XMIN], o[YMIN], o[XMAX], o[YMAX] = min(o[XMIN], x), min(o[YMIN], y), max(o[XMAX], x), max(o[YMAX], y)
            o[SUMX] += x
            o[SUMY] += y
            if any(0 <= yy < h and 0 <= xx < w and label_of(yy, xx) != lab for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1))):
                o[EDGE] += 1
            if y in (0, h - 1) or x in (0, w - 1):
                o[BORDER] += 1
            if stack:
                o[CONF] += _q1(answer[s, y, x])
    return np.array(out, dtype=np.int64)


def report(answers, ids):
    """n frames -> (n, 16, 12) int64."""
    return np.stack([words(a, i) for a, i in zip(answers, ids)])


def blob_labels(rng, h, w, ids):
    """Blobs of a few pixels, each one of ``ids``, so that objects have boundaries."""
    bh, bw = max(1, h // 4), max(1, w // 6)
    owner = rng.integers(0, len(ids), ((h + bh - 1) // bh, (w + bw - 1) // bw))
    return np.asarray(ids, dtype=np.uint8)[np.kron(owner, np.ones((bh, bw), dtype=np.int64))[:h, :w]]


def merged_stack(rng, K, h, w):
    """A merged-like (K, h, w) float32 stack: one plane nonzero per pixel, its value uniform in (0, 1), in blobs."""
    bh, bw = max(1, h // 5), max(1, w // 7)
    owner = rng.integers(0, K, ((h + bh - 1) // bh, (w + bw - 1) // bw))
    owner = np.kron(owner, np.ones((bh, bw), dtype=np.int64))[:h, :w]
    val = rng.uniform(0.05, 1.0, (h, w)).astype(np.float32)
    return np.where(owner[None] == np.arange(K)[:, None, None], val[None], np.float32(0)).astype(np.float32)


# the stack values the decode and q can get wrong: name -> {plane: value} (the other planes of the pixel are 0); `planes`: the K it needs
HAND = [
    ('half_is_background', 2, {1: 0.5}),
    ('tie_first_wins', 3, {1: 0.75, 2: 0.75}),
    ('nan_next_to_finite', 3, {1: np.nan, 2: 0.625}),
    ('nans_only', 1, None),                                             # every plane of the pixel a NaN
    ('above_one', 2, {1: 1.5}),
    ('below_zero', 2, {1: -0.25}),
    ('background_above_an_object', 3, {0: 0.9, 1: 0.75, 2: 0.8}),
]


def hand_placed(stack):
    """The HAND pixels written over the LAST pixels of the picture, as many as it has room and planes for -> (stack, names placed)."""
    K, h, w = stack.shape
    flat = stack.reshape(K, -1)
    placed = []
    for name, planes, case in HAND:
        if planes > K or len(placed) >= h * w:
            continue
        i = h * w - 1 - len(placed)
        flat[:, i] = np.nan if case is None else 0
        for k, v in (case or {}).items():
            flat[k, i] = v
        placed.append(name)
    return stack, placed
