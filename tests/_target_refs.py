"""Plain torch definitions of the memory and gradient half of csrc/target_model.hip -- what feeds the solver: pixel weights, the low-resolution
normal equations, the sample-weight and slot logic of the memory, the stand-alone mask merge -- written from the contracts of
include/frtm_hip.h with no project code.  The filter gradients, the stencil and the 3x3 scores are those of tests/_solver_refs.py and are
imported, not restated.  Every function works in the dtype and on the device of its arguments, so the same text serves as the float64
reference on the CPU and as the fp32 yardstick of the gate on the GPU.  tests/test_target_refs.py pins them to oracle/cpu_ref.py.

Layouts are those of the C side: labels and pixel weights (n, H, W); B (n, 9, h, w) with tap (a, b) = plane 3 a + b coupling cell (ci, cj) with
cell (ci + a - 1, cj + b - 1); c (n, h, w); sample weights (cap); the slot state as four integers {previous slot or -1, slot of this call or
-1, inserts performed, inserts skipped}; mask planes (..., K, HW).

The input makers of the GPU tests whose conditions tests/test_target_refs.py asserts on the CPU (the merge cases and their margin share, the
9 / 10 pixel hinge boundary) live here as well, so that both modules see the same values.
"""
import os
import sys

import torch
import torch.nn.functional as F

from _solver_refs import conv3x3, filter_igrad, filter_wgrad, stencil  # noqa: F401  (the one definition of each; re-exported)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle.cpu_ref import bilinear_matrix  # noqa: E402

PX_PARTS = 32                                                     # FRTM_PX_PARTS
MERGE_MAX = 16                                                    # planes k_merge_masks holds per thread; above: k_merge_masks_any
MERGE_LO = float(torch.tensor(1e-7, dtype=torch.float32))         # the merge's clamp bounds as the fp32 values the kernel holds
MERGE_HI = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(1e-7, dtype=torch.float32))
WINNER_MARGIN = 2.0 ** -20                                        # relative margin of the two largest odds above which the winner is asserted
LR = float(torch.tensor(0.1, dtype=torch.float32))                # the memory's learning rate as the fp32 value the kernel is handed


# ---------------------------------------------------------------------------------------------------------------------------------
# pixel weights
# ---------------------------------------------------------------------------------------------------------------------------------
def hinge(px, HW, tf):
    """hinge_weights of target_model.hip.  px: tensor of foreground pixel counts (any shape) -> (wf, wb) of that shape.
    tf < 0: both 1.  af = px / HW, replaced by tf where px < 10; tfe = max(af, tf); wf = tfe / af; wb = (1 - tfe) / (1 - af)."""
    if tf < 0:
        return torch.ones_like(px), torch.ones_like(px)
    tft = torch.full_like(px, tf)
    af = px / HW
    af = torch.where(px < 10, tft, af)
    tfe = torch.where(af > tf, af, tft)
    return tfe / af, (1 - tfe) / (1 - af)


def pixel_weights(y, tf):
    """frtm_pixel_weights.  y (n, H, W) with values in {0, 1} -> sqrt(wf y + wb (1 - y)), the count being the plain sum of y (the kernel sums
    the raw label values, it does not threshold them: for labels in {0, 1} the two are one)."""
    n, H, W = y.shape
    wf, wb = hinge(y.sum(dim=(1, 2)), H * W, tf)
    return torch.sqrt(wf.view(n, 1, 1) * y + wb.view(n, 1, 1) * (1 - y))


# ---------------------------------------------------------------------------------------------------------------------------------
# low-resolution normal equations
# ---------------------------------------------------------------------------------------------------------------------------------
def normals(labels, pw, px, h, w, tf):
    """frtm_normal_build.  labels (n, H, W) (soft or {0, 1}); pw (n, H, W) explicit pixel weights or None (hinge weights of ys = labels > 0.5
    with the count px (n), None: the number of pixels > 0.5) -> B (n, 9, h, w), c (n, h, w):
        B[(a,b)][ci,cj] = sum_{Y,X} m(Y,X) Wy[Y,ci] Wx[X,cj] Wy[Y,ci+a-1] Wx[X,cj+b-1]   (taps outside the grid: 0)
        c[ci,cj]        = sum_{Y,X} m(Y,X) Wy[Y,ci] Wx[X,cj] label(Y,X)
    with m = pw^2, or wf ys + wb (1 - ys), and Wy (H, h), Wx (W, w) the dense ATen bilinear matrices (align_corners=False).  The sums run over
    all pixels of the image: no window."""
    n, H, W = labels.shape
    dt, dev = labels.dtype, labels.device
    Wy, Wx = bilinear_matrix(h, H, dt).to(dev), bilinear_matrix(w, W, dt).to(dev)
    if pw is not None:
        m = pw * pw
    else:
        ys = (labels > 0.5).to(dt)
        cnt = ys.sum(dim=(1, 2)) if px is None else px.to(dt)
        wf, wb = hinge(cnt, H * W, tf)
        m = wf.view(n, 1, 1) * ys + wb.view(n, 1, 1) * (1 - ys)
    Wyp, Wxp = F.pad(Wy, (1, 1)), F.pad(Wx, (1, 1))                # column k + 1 = cell k; cells -1 and h (w): zero
    B = labels.new_zeros(n, 9, h, w)
    for a in range(3):
        Py = Wy * Wyp[:, a:a + h]
        for b in range(3):
            B[:, a * 3 + b] = torch.einsum('Yi,nYX,Xj->nij', Py, m, Wx * Wxp[:, b:b + w])
    return B, torch.einsum('Yi,nYX,Xj->nij', Wy, m * labels, Wx)


# ---------------------------------------------------------------------------------------------------------------------------------
# sample weights and slots
# ---------------------------------------------------------------------------------------------------------------------------------
def next_slot(sw, lr, num_zero, state, count, min_count):
    """One call of next_slot_step (frtm_memory_next_slot), state in and state out: -> (sw, state, slot).  sw (cap); state: four integers;
    count: an integer or None.  count < min_count: nothing but state[1] = -1 and state[3] += 1.  Else num_zero or lr == 1: sw = e_0, slot 0;
    otherwise the slot is the arg-min of sw (ties: the lowest index) and, with no previous slot (state[0] < 0), sw /= 1 - lr, sw[slot] = lr,
    with one, sw[slot] = sw[state[0]] / (1 - lr); then sw /= sum(sw), state[0] = state[1] = slot, state[2] += 1."""
    sw, st = sw.clone(), [int(v) for v in state]
    if count is not None and int(count) < min_count:
        st[1] = -1
        st[3] += 1
        return sw, st, -1
    if num_zero or lr == 1:
        sw.zero_()
        sw[0] = 1
        r = 0
    else:
        r = int((sw == sw.min()).nonzero()[0])
        if st[0] < 0:
            sw = sw / (1 - lr)
            sw[r] = lr
        else:
            sw[r] = sw[st[0]] / (1 - lr)
    sw = sw / sw.sum()
    st[0], st[1] = r, r
    st[2] += 1
    return sw, st, r


def window(sw, lr, num_zero, state, counts, min_count):
    """next_slot applied once per entry of `counts`, one after the other (k_memory_next_slot_window) -> (sw, state, slots); after the first
    insert that was performed the memory is no longer empty."""
    slots = []
    for cnt in counts:
        sw, state, r = next_slot(sw, lr, num_zero, state, cnt, min_count)
        if r >= 0:
            num_zero = 0
        slots.append(r)
    return sw, state, slots


# ---------------------------------------------------------------------------------------------------------------------------------
# mask merge
# ---------------------------------------------------------------------------------------------------------------------------------
def merge(masks):
    """frtm_merge_masks(_frames).  masks (..., K, HW) -> (out, arg, margin): p = clamp(masks, 1e-7, 1 - 1e-7) (the bounds as fp32 holds them);
    p[0] = min_k>0 (1 - p[k]); odds o = p / (1 - p); arg = the first plane of the largest odds; out[arg] = softmax(o)[arg], every other plane 0.
    margin (..., HW): (largest - second largest odds) / largest."""
    K = masks.shape[-2]
    p = torch.clamp(masks, MERGE_LO, MERGE_HI)
    p = torch.cat([(1 - p[..., 1:, :]).min(dim=-2, keepdim=True)[0], p[..., 1:, :]], dim=-2)
    o = p / (1 - p)
    mx, arg = o[..., 0, :].clone(), torch.zeros(o.shape[:-2] + o.shape[-1:], dtype=torch.int64, device=o.device)
    for k in range(1, K):
        better = o[..., k, :] > mx
        mx = torch.where(better, o[..., k, :], mx)
        arg = torch.where(better, torch.full_like(arg, k), arg)
    e = torch.exp(o - mx.unsqueeze(-2))
    win = 1.0 / e.sum(dim=-2)                                     # exp(0) / den
    out = torch.zeros_like(masks).scatter_(-2, arg.unsqueeze(-2), win.unsqueeze(-2))
    top2 = torch.topk(o, 2, dim=-2)[0]
    return out, arg, (top2[..., 0, :] - top2[..., 1, :]) / top2[..., 0, :]


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs shared by tests/test_target_refs.py (conditions, CPU) and tests/test_target_data_gpu.py
# ---------------------------------------------------------------------------------------------------------------------------------
MERGE_CASES = [(K, HW, fr) for K in (2, 3, 16, 17, 20) for HW in (1, 255, 70000) for fr in (1, 3)]


def merge_input(K, HW, frames):
    """-> (masks (frames, K, HW) fp32, ties): uniform values in [-0.1, 1.1]; from 255 pixels on, in every frame, pixel 0 holds 0 in plane 1,
    pixel 1 holds 1 in plane 1, pixel 2 holds 0.5 in plane K - 1 with every other object below 0.5 (background and that object both have odds
    1: plane 0 wins) and, with K >= 3, pixel 3 holds 0.75 in planes 1 and 2 with every other object below (odds 3 twice: plane 1 wins).
    ties: {pixel: winning plane} of the planted exact ties.  Plane 0 of the input is never read."""
    g = torch.Generator().manual_seed(7000 + 100 * K + frames + HW % 97)
    m = torch.rand(frames, K, HW, generator=g) * 1.2 - 0.1
    ties = {}
    if HW >= 255:
        m[:, 1, 0] = 0.0
        m[:, 1, 1] = 1.0
        m[:, 1:, 2] = m[:, 1:, 2].clamp(0.0, 1.0) * 0.4
        m[:, K - 1, 2] = 0.5
        ties[2] = 0
        if K >= 3:
            m[:, 1:, 3] = m[:, 1:, 3].clamp(0.0, 1.0) * 0.7
            m[:, 1, 3] = 0.75
            m[:, 2, 3] = 0.75
            ties[3] = 1
    return m, ties


def merge_checked(margin):
    """The pixels at which the winning plane is asserted: relative margin above WINNER_MARGIN, or exactly 0.  A float64 margin of 0 on fp32
    inputs is an exact tie in fp32 as well -- two objects clamped to the same bound, the planted 0.75 pair, an object equal to 1 - the largest
    one (1 - p is exact where its result is an fp32 value) -- so the tie rule decides there: the first plane.  Left out: 0 < margin <= 2^-20."""
    return (margin > WINNER_MARGIN) | (margin == 0)


def labels_with_count(H, W, count, seed):
    """(H, W) fp32 labels in {0, 1} with exactly `count` ones at seeded places."""
    g = torch.Generator().manual_seed(seed)
    y = torch.zeros(H * W)
    y[torch.randperm(H * W, generator=g)[:count]] = 1.0
    return y.view(H, W)


def boundary_tf(HW):
    """A tf at which 9 and 10 foreground pixels of HW fall on different sides of the `px < 10` rule with different weights: above 10 / HW (at 10
    pixels af = 10 / HW < tf, so wf = tf / af != 1, at 9 pixels af = tf and both weights are 1)."""
    return 0.1 if 10.0 / HW < 0.05 else (0.25 if 10.0 / HW < 0.2 else 0.75)
