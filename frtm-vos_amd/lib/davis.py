"""DAVIS region (J) and boundary (F) measures (names of the reference's lib/davis.py:19-189, itself a port of the public
DAVIS toolkit; that file cannot run here: it needs skimage and uses np.bool, removed in numpy >= 1.24).

Restated from the published definitions (Perazzi et al., CVPR 2016):
  J  = |M & G| / |M | G|  (1 when both are empty)
  F  = 2PR/(P+R) between the boundary maps of M and G, a boundary pixel counting as matched when the other boundary has
       a pixel within bound_th * image diagonal (>= 1 px), implemented as a disk dilation.
Pixel-exact agreement with skimage's disk()/binary_dilation is UNPINNED (skimage is not installed); the disk here is
{(dy,dx): dy^2 + dx^2 <= r^2}.

Both measures are functions of six integers per (frame, object) -- inter, union, n_fg, n_gt, fg_match, gt_match -- and there is one
place that knows those functions: iou_from_counts / f_from_counts.  numpy arrays and CPU tensors are counted here with numpy / scipy;
label maps that are CUDA tensors are counted by the HIP kernels of csrc/jf_eval.hip (ops.jf_counts: every frame and object of a
sequence in one call, one device-to-host read), which gives the same integers and therefore bit-identical J and F.
"""
import numpy as np
from scipy import ndimage

COUNT_NAMES = ('inter', 'union', 'n_fg', 'n_gt', 'fg_match', 'gt_match')          # last axis of ops.jf_counts / device_counts


def iou_from_counts(inter, union):
    """J from |M & G| and |M | G| (1 when both are empty)."""
    if union == 0:
        return 1.0
    return float(inter) / float(union)


def f_from_counts(n_fg, n_gt, fg_match, gt_match):
    """F from the boundary pixel counts of prediction and ground truth and how many of each have a pixel of the other boundary within
    the disk (the matches are not looked at when either boundary is empty)."""
    if n_fg == 0 and n_gt > 0:
        precision, recall = 1.0, 0.0
    elif n_fg > 0 and n_gt == 0:
        precision, recall = 0.0, 1.0
    elif n_fg == 0 and n_gt == 0:
        precision, recall = 1.0, 1.0
    else:
        precision, recall = fg_match / float(n_fg), gt_match / float(n_gt)
    if precision + recall == 0:
        return 0.0
    return float(2 * precision * recall / (precision + recall))


def boundary_radius(shape, bound_th=0.008):
    """Radius of the matching disk in pixels: bound_th itself when >= 1, else that fraction of the image diagonal, rounded up; >= 1."""
    bound_pix = bound_th if bound_th >= 1 else int(np.ceil(bound_th * np.linalg.norm(shape)))
    return max(int(bound_pix), 1)


def db_eval_iou(annotation, segmentation):
    a = np.asarray(annotation).astype(bool)
    s = np.asarray(segmentation).astype(bool)
    return iou_from_counts(int(np.logical_and(a, s).sum()), int(np.logical_or(a, s).sum()))


def seg2bmap(seg):
    """Boundary map: a pixel is a boundary pixel if it differs from its east, south or south-east neighbour."""
    seg = np.asarray(seg).astype(bool)
    e = np.zeros_like(seg)
    s = np.zeros_like(seg)
    se = np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    e[:, -1] = seg[:, -1]
    s[:-1, :] = seg[1:, :]
    s[-1, :] = seg[-1, :]
    se[:-1, :-1] = seg[1:, 1:]
    se[:-1, -1] = seg[1:, -1]
    se[-1, :-1] = seg[-1, 1:]
    se[-1, -1] = seg[-1, -1]
    b = (seg ^ e) | (seg ^ s) | (seg ^ se)
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = False
    return b


def _disk(r):
    y, x = np.ogrid[-r:r + 1, -r:r + 1]
    return (x * x + y * y) <= r * r


def _within(points, of, r):
    """Which `points` pixels have an `of` pixel within the disk {dy^2 + dx^2 <= r^2}: exactly `points & binary_dilation(of, _disk(r))`
    (zero border), through one exact Euclidean distance transform instead of a (2r+1)^2-element dilation -- 17x17 at 480p, where the
    dilation took ~0.1 s per map and made the boundary measure the cost of every dataset evaluation (of needs at least one pixel)."""
    ys, xs = np.flatnonzero(of.any(1)), np.flatnonzero(of.any(0))
    y0, y1 = max(int(ys[0]) - r, 0), min(int(ys[-1]) + r + 1, of.shape[0])         # nothing outside the bounding box of `of` grown by r can match
    x0, x1 = max(int(xs[0]) - r, 0), min(int(xs[-1]) + r + 1, of.shape[1])
    d = ndimage.distance_transform_edt(~of[y0:y1, x0:x1])   # sqrt of the exact integer squared distance: d <= r  <=>  dy^2 + dx^2 <= r^2
    out = np.zeros_like(points)
    out[y0:y1, x0:x1] = points[y0:y1, x0:x1] & (d <= r)
    return out


def db_eval_boundary(foreground_mask, gt_mask, bound_th=0.008):
    fg = np.asarray(foreground_mask).astype(bool)
    gt = np.asarray(gt_mask).astype(bool)
    return f_from_counts(*boundary_counts(fg, gt, boundary_radius(fg.shape, bound_th)))


def boundary_counts(fg, gt, r):
    """(n_fg, n_gt, fg_match, gt_match) of two boolean masks with numpy / scipy; the matches stay 0 when either boundary is empty
    (f_from_counts does not read them then)."""
    fg_b, gt_b = seg2bmap(fg), seg2bmap(gt)
    n_fg, n_gt = int(fg_b.sum()), int(gt_b.sum())
    if n_fg == 0 or n_gt == 0:
        return n_fg, n_gt, 0, 0
    return n_fg, n_gt, int(_within(fg_b, gt_b, r).sum()), int(_within(gt_b, fg_b, r).sum())


# ---- label maps on the GPU: the counts come from the HIP kernels (ops.jf_counts) ---------------------------------------------

def _is_cuda(v):
    return bool(getattr(v, 'is_cuda', False))


def on_device(*label_sets):
    """True when the label maps handed in (per set: one tensor, or a list of per-frame maps) are CUDA tensors, i.e. the counts are to
    come from the GPU.  A mixture of CUDA tensors and anything else is refused: nothing is copied between devices behind the caller."""
    flags = []
    for s in label_sets:
        flags.extend([_is_cuda(s)] if (_is_cuda(s) or not isinstance(s, (list, tuple))) else [_is_cuda(v) for v in s])
    if any(flags) and not all(flags):
        raise ValueError('J / F evaluation: some label maps are CUDA tensors and some are not; pass all of them on one GPU, or all as '
                         'numpy arrays / CPU tensors')
    return bool(flags) and all(flags)


def _stack_labels(labels, what):
    """Per-frame maps ((1,H,W) or (H,W) each) or one (T,H,W) / (T,1,H,W) tensor -> one dense (T,H,W) device tensor, uint8 or int32.
    A list is gathered with device-to-device copies (no framework kernel)."""
    import torch
    if _is_cuda(labels):
        t = labels
        if t.dim() == 4 and t.shape[1] == 1:
            t = t.reshape(t.shape[0], t.shape[2], t.shape[3])
        if t.dim() != 3:
            raise ValueError('J / F evaluation: %s must be (T,H,W) or (T,1,H,W), got %s' % (what, tuple(labels.shape)))
    else:
        first = labels[0]
        if first.dim() < 2:
            raise ValueError('J / F evaluation: %s frames must be (H,W) or (1,H,W), got %s' % (what, tuple(first.shape)))
        hw = tuple(first.shape[-2:])
        for v in labels:
            if v.device != first.device:
                raise ValueError('J / F evaluation: %s frames on %s and %s' % (what, first.device, v.device))
            if v.dtype != first.dtype:
                raise TypeError('J / F evaluation: %s frames of %s and %s' % (what, first.dtype, v.dtype))
            if tuple(v.shape[-2:]) != hw or v.numel() != hw[0] * hw[1]:
                raise ValueError('J / F evaluation: %s frames of shape %s and %s' % (what, tuple(first.shape), tuple(v.shape)))
        n, store = hw[0] * hw[1], first.untyped_storage().data_ptr()
        if all(v.is_contiguous() and v.untyped_storage().data_ptr() == store and v.storage_offset() == first.storage_offset() + i * n
               for i, v in enumerate(labels)):
            # consecutive slices of one tensor (Tracker.run_sequence's list, a pre-loaded sequence's ground truth): a view, nothing to copy
            t = torch.as_strided(first, (len(labels),) + hw, (n, hw[1], 1))
        else:
            t = torch.empty((len(labels),) + hw, dtype=first.dtype, device=first.device)
            for i, v in enumerate(labels):
                t[i].copy_(v.contiguous().view(hw))
    if t.dtype.is_floating_point or t.dtype.is_complex:
        raise TypeError('J / F evaluation: %s label maps must be integer tensors, got %s' % (what, t.dtype))
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype not in (torch.uint8, torch.int32):
        t = t.to(torch.int32)
    return t.contiguous()


def device_counts(pred_labels, gt_labels, obj_ids, bound_th=0.008):
    """(T,K,6) int64 numpy array of COUNT_NAMES for every frame and object id of a sequence whose label maps are on the GPU: one call
    of ops.jf_counts, one device-to-host read."""
    import torch
    from .. import ops
    pred, truth = _stack_labels(pred_labels, 'predicted'), _stack_labels(gt_labels, 'ground-truth')
    if pred.device != truth.device:
        raise ValueError('J / F evaluation: predictions on %s, ground truth on %s' % (pred.device, truth.device))
    if pred.shape != truth.shape:
        raise ValueError('J / F evaluation: predictions %s and ground truth %s differ in shape' % (tuple(pred.shape), tuple(truth.shape)))
    if pred.dtype != truth.dtype:
        pred, truth = pred.to(torch.int32), truth.to(torch.int32)
    r = boundary_radius(tuple(pred.shape[-2:]), bound_th)
    if r > ops.JF_MAX_RADIUS:
        raise ValueError('J / F evaluation on the GPU covers matching radii up to %d px, this one is %d px (%s frame, bound_th %g): use the '
                         'numpy path (pass numpy arrays or CPU tensors)' % (ops.JF_MAX_RADIUS, r, 'x'.join(str(v) for v in pred.shape[-2:]), bound_th))
    with torch.cuda.device(pred.device):
        return ops.jf_counts(pred, truth, list(obj_ids), r).cpu().numpy().astype(np.int64)


def measure_from_counts(c, measure):
    """J or F of one (frame, object) from its row of COUNT_NAMES (prediction = foreground)."""
    inter, union, n_fg, n_gt, fg_match, gt_match = (int(v) for v in c)
    return iou_from_counts(inter, union) if measure == 'J' else f_from_counts(n_fg, n_gt, fg_match, gt_match)


def db_statistics(per_frame_values):
    """Mean, recall (fraction > 0.5) and decay (first-quarter mean minus last-quarter mean) over the frames."""
    v = np.asarray(per_frame_values, dtype=np.float64)
    v = v[~np.isnan(v)]
    if v.size == 0:
        return float('nan'), float('nan'), float('nan')
    ids = np.round(np.linspace(1, len(v), 5) + 1e-10).astype(np.int64) - 1
    bins = [v[ids[i]:ids[i + 1] + 1] for i in range(4)]
    return float(v.mean()), float((v > 0.5).mean()), float(np.mean(bins[0]) - np.mean(bins[3]))


# ---- the reference's names (lib/davis.py:19-236), pinned by tests/golden/g10_davis.npz --------------------------------------

def davis_jaccard_measure(fg_mask, gt_mask):
    """Reference lib/davis.py:54-71 (argument order: segmentation first)."""
    return db_eval_iou(gt_mask, fg_mask)


def davis_f_measure(foreground_mask, gt_mask, bound_th=0.008):
    """Reference lib/davis.py:75-131."""
    return db_eval_boundary(foreground_mask, gt_mask, bound_th)


def nanmean(*args, **kwargs):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', category=RuntimeWarning)
        return np.nanmean(*args, **kwargs)


def mean(X):
    return nanmean(np.asarray(X, dtype=np.float64))


def std(X):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', category=RuntimeWarning)
        return np.nanstd(np.asarray(X, dtype=np.float64))


def recall(X, threshold=0.5):
    x = np.asarray(X, dtype=np.float64)
    x = x[~np.isnan(x)]
    return nanmean(x > threshold) if x.size else float('nan')


def decay(X, n_bins=4):
    """First-quarter mean minus last-quarter mean over the non-NaN values (reference lib/davis.py:214-227; the bin edges go
    through uint8 there, so sequences beyond 256 evaluated frames wrap -- kept: DAVIS / YouTube-VOS sequences are shorter)."""
    x = np.asarray(X, dtype=np.float64)
    x = x[~np.isnan(x)]
    ids = (np.round(np.linspace(1, len(x), n_bins + 1) + 1e-10) - 1).astype(np.uint8)
    bins = [x[ids[i]:ids[i + 1] + 1] for i in range(4)]
    return nanmean(bins[0]) - nanmean(bins[3])


def evaluate_sequence(segmentations, annotations, object_info, measure='J'):
    """Reference lib/davis.py:19-50.  segmentations / annotations: ordered dicts frame name -> label image ((1,H,W) tensor or
    (H,W) array); object_info: {object id: name of its first frame}.  A frame counts for an object strictly after the
    object's first frame and strictly before the last frame of the sequence; the others stay NaN."""
    fn = {'J': davis_jaccard_measure, 'F': davis_f_measure}[measure]
    names = list(annotations.keys())
    if on_device(list(segmentations.values()), list(annotations.values())):
        counts = device_counts(list(segmentations.values()), list(annotations.values()), list(object_info.keys()))
        return sequence_from_counts(counts, names, object_info, measure)
    out = dict(raw={})

    def arr(v):
        v = v.numpy() if hasattr(v, 'numpy') else np.asarray(v)
        return v.reshape(v.shape[-2:])
    for obj_id, first in object_info.items():
        r = np.full(len(names), np.nan)
        i0 = names.index(first)
        for i, (an, sg) in enumerate(zip(annotations, segmentations)):
            if i0 < i < len(names) - 1:
                r[i] = fn(arr(segmentations[sg]) == obj_id, arr(annotations[an]) == obj_id)
        out['raw'][obj_id] = r
    return _with_statistics(out)


def sequence_from_counts(counts, names, object_info, measure='J'):
    """evaluate_sequence from the (T,K,6) counts of device_counts (object k = the k-th key of object_info): same frame selection, same
    statistics."""
    assert measure in ('J', 'F') and counts.shape[:2] == (len(names), len(object_info))
    out = dict(raw={})
    for k, (obj_id, first) in enumerate(object_info.items()):
        r = np.full(len(names), np.nan)
        i0 = names.index(first)
        for i in range(i0 + 1, len(names) - 1):
            r[i] = measure_from_counts(counts[i, k], measure)
        out['raw'][obj_id] = r
    return _with_statistics(out)


def _with_statistics(out):
    for name, f in (('decay', decay), ('mean', mean), ('recall', recall), ('std', std)):
        out[name] = [float(f(r)) for r in out['raw'].values()]
    return out
