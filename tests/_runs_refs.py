"""The run-length coding of csrc/mask_runs.hip stated twice: in numpy (``counts``: flatten(order='F'), diff) and as a plain loop over pixels
(``counts_loop``, which checks the numpy statement), with the slot rule of include/frtm_hip.h, COCO's string form and the layout of
``heads`` / ``runs``.  Everything is an exact integer function of the inputs, so the tests compare with ``==``.  Self-contained: the decode
and the string codec are restated here, not imported.

    slot:    stack: arg = the first k with the largest m_k (a NaN never wins); arg if arg >= 1 and m_arg > 0.5f, else 0
             label map: the index of the pixel's id in ``ids`` (the first, if listed twice), none when not listed
    counts:  the lengths of the maximal runs of equal bits of b_s(p), p = x h + y, starting with a run of ZEROS (0 when b_s(0) = 1)
    heads:   per frame 16 x { count, offset, area, id }; offsets run on over (frame, slot); slots >= K: zeros
    runs:    the concatenation; element j is stored iff j < capacity"""
import numpy as np

SLOTS, HEAD = 16, 4
COUNT, OFFSET, AREA, ID = range(4)


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


def counts(mask):
    """The run lengths of a (h, w) bool mask, vectorised."""
    bits = np.asarray(mask, dtype=bool).flatten(order='F')
    edges = np.flatnonzero(np.diff(bits.astype(np.int8))) + 1            # the positions p >= 1 where the bit changes
    pos = np.concatenate([[0], edges, [bits.size]])
    runs = np.diff(pos).tolist()
    return [0] + runs if bits[0] else runs


def counts_loop(mask):
    """``counts`` as a loop over pixels in plain Python."""
    mask = np.asarray(mask)
    h, w = mask.shape
    out, bit, run = [], 0, 0
    for x in range(w):
        for y in range(h):
            b = 1 if mask[y, x] else 0
            if b != bit:
                out.append(run)
                bit, run = b, 0
            run += 1
    out.append(run)
    return out


def decode_counts(size, c):
    """The (h, w) bool mask of a list of run lengths, as a loop."""
    h, w = size
    flat, bit = [], False
    for r in c:
        flat += [bit] * int(r)
        bit = not bit
    assert len(flat) == h * w
    return np.array(flat, dtype=bool).reshape(w, h).T


def to_string(c):
    """COCO's string form (the issue's statement of it)."""
    out = bytearray()
    for i, x in enumerate(int(v) for v in c):
        if i > 2:
            x -= int(c[i - 2])
        while True:
            g = x & 0x1f
            x >>= 5
            done = (x == -1) if g & 0x10 else (x == 0)
            out.append(g + 48 if done else (g | 0x20) + 48)
            if done:
                break
    return bytes(out)


def frame_counts(answer, ids):
    """One frame -> [counts of slot s for s < K]."""
    slot = slots(answer, ids)
    return [counts(slot == s) for s in range(len(np.asarray(ids).reshape(-1)))]


def layout(answers, ids, capacity=None):
    """n frames -> (heads (n, 16, 4) int64, runs int64: the concatenation cut at ``capacity``, needed)."""
    heads = np.zeros((len(answers), SLOTS, HEAD), dtype=np.int64)
    cat, off = [], 0
    for f, (a, i) in enumerate(zip(answers, ids)):
        idv = [int(v) for v in np.asarray(i).reshape(-1)]
        for s, c in enumerate(frame_counts(a, idv)):
            heads[f, s] = (len(c), off, sum(c[1::2]), idv[s])
            cat += c
            off += len(c)
    runs = np.array(cat, dtype=np.int64)
    return heads, runs if capacity is None else runs[:capacity], off


def blob_labels(rng, h, w, ids):
    """Blobs of a few pixels, each one of ``ids``, so that objects have boundaries."""
    bh, bw = max(1, h // 4), max(1, w // 6)
    owner = rng.integers(0, len(ids), ((h + bh - 1) // bh, (w + bw - 1) // bw))
    return np.asarray(ids, dtype=np.uint8)[np.kron(owner, np.ones((bh, bw), dtype=np.int64))[:h, :w]]


def stack_of(planes, K, rng=None):
    """A merged-like (K, h, w) float32 stack whose decoded plane is ``planes`` (values 0 .. K - 1): the owner's plane holds a value above
    0.5 (0.75, or uniform in (0.51, 1) with ``rng``), every other plane 0."""
    planes = np.asarray(planes)
    val = np.full(planes.shape, 0.75, dtype=np.float32) if rng is None else rng.uniform(0.51, 1.0, planes.shape).astype(np.float32)
    return np.where(planes[None] == np.arange(K)[:, None, None], val[None], np.float32(0)).astype(np.float32)
