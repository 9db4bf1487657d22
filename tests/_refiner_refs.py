"""Plain torch definitions of the refiner's element-wise kernels (csrc/refiner_ops.hip, csrc/refiner_train.hip), one per kernel.

Written from the modules of model/seg_network.py (TSE, CAB, BackwardCompatibleUpsampler) as SegNetwork.forward_torch composes them, with no
project code: the forward ones are closed expressions (F.interpolate, F.conv2d, matrix products, torch.sigmoid), the backward ones
torch.autograd.grad of those expressions.  Every function works in the dtype and on the device of its arguments, so the same text serves
as the float64 reference and as the fp32 yardstick of the gate.  tests/test_refiner_kernels.py pins them to the float64 modules.

Argument layouts are those of the C entry points (include/frtm_hip.h): planes flattened, W1 / W2 of the forward gate as [in][out], of the
backward gate in the conv layout [out][in].
"""
import torch
import torch.nn.functional as F


def _cubic(x, a=-0.75):
    """The cubic-convolution kernel (Keys, a = -0.75) at distance x >= 0."""
    if x <= 1:
        return (a + 2) * x ** 3 - (a + 3) * x ** 2 + 1
    if x < 2:
        return a * x ** 3 - 5 * a * x ** 2 + 8 * a * x - 4 * a
    return 0.0


# taps of the two phases of the 2x polyphase up-sampling: sub-pixel offsets -0.25 and -0.75 (all eight are multiples of 1 / 256)
PYR_TAPS = [[_cubic(abs(d + k)) for k in range(-1, 3)] for d in (-0.25, -0.75)]


def _resize(x, H, W):
    """(n,c,h,w) -> (n,c,H,W): bilinear, align_corners=False; the identity when the size agrees (lib/utils.py: interpolate)."""
    if tuple(x.shape[-2:]) == (H, W):
        return x
    return F.interpolate(x, (H, W), mode='bilinear', align_corners=False)


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
def bilinear_resize(x, H, W):
    """k_bilinear_resize.  x (planes,h,w) -> (planes,H,W)."""
    return F.interpolate(x[None], (H, W), mode='bilinear', align_corners=False)[0]


def _pyrup_last(x):
    """2x along the last axis: replicate pad 2, both phases as a 4-tap correlation, interleave, crop one sample at either end."""
    L = x.shape[-1]
    k = torch.tensor(PYR_TAPS, dtype=x.dtype, device=x.device)
    xp = F.pad(x.reshape(-1, 1, 1, L), (2, 2, 0, 0), mode='replicate')
    y = F.conv2d(xp, k.view(2, 1, 1, 4))                               # (P, 2, 1, L + 1)
    y = y.permute(0, 2, 3, 1).reshape(-1, 2 * (L + 1))[:, 1:-1]
    return y.reshape(*x.shape[:-1], 2 * L)


def pyrup2x(x):
    """k_pyrup2x.  x (planes,h,w) -> (planes,2h,2w): PyrUpBicubic2d, rows then columns."""
    y = _pyrup_last(x.transpose(-1, -2).contiguous()).transpose(-1, -2).contiguous()
    return _pyrup_last(y)


def plane_mean(x):
    """k_plane_mean.  x (planes,HW) -> (planes,): adaptive_avg_pool2d to 1x1."""
    return x.mean(1)


def tse_inject(base, bias, ws, scores, group):
    """k_tse_inject.  base (frames,C,H,W): transform[0]'s 3x3 conv over the feature channels, no bias; ws (C,9): its weights on the score
    channel; scores (n,h,w), n = frames * group, frame-major.  Returns relu(transform[0](cat(h, interpolate(score)))) (n,C,H,W)."""
    C, H, W = base.shape[1:]
    s = _resize(scores[:, None], H, W)
    return F.relu(base.repeat_interleave(group, 0) + bias.view(1, C, 1, 1) + F.conv2d(s, ws.view(C, 1, 3, 3), padding=1))


def cab_gate(sp, dp, dp_group, W1, b1, W2, b2):
    """k_cab_gate.  sp (n,oc), dp (n,oc) or, with dp_group > 0, (n / dp_group, oc); W1 (2oc,oc), W2 (oc,oc) as [in][out].
    Returns convreluconv(cat(shallow_pool, deeper_pool)) (n,oc), before the sigmoid."""
    d = dp.repeat_interleave(dp_group, 0) if dp_group > 0 else dp
    return torch.matmul(F.relu(torch.matmul(torch.cat((sp, d), 1), W1) + b1), W2) + b2


def cab_combine(shallow, gate, deeper, deeper_group):
    """k_cab_combine.  shallow (n,C,H,W), gate (n,C), deeper (n or n / deeper_group, C, hd, wd).
    Returns shallower * sigmoid(gate) + interpolate(deeper)."""
    d = deeper.repeat_interleave(deeper_group, 0) if deeper_group > 0 else deeper
    return shallow * torch.sigmoid(gate)[:, :, None, None] + _resize(d, shallow.shape[2], shallow.shape[3])


def tap_mix(y, w):
    """k_tap_mix.  y (n,C,hw), w (C,9) -> (n,9,hw): Y_t = sum_c w[c,t] y_c."""
    return torch.matmul(w.t(), y)


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
def _grad(out, wrt, upstream):
    return torch.autograd.grad(out, wrt, upstream, allow_unused=False)


def relu_backward(dy, y):
    """k_relu_bwd: the gradient of relu, taken at the saved output (relu(y) = y there; 0 at 0 and at -0.0)."""
    with torch.enable_grad():
        x = y.detach().clone().requires_grad_()
        return _grad(F.relu(x), [x], dy)[0]


def shift9(dl):
    """k_shift9.  dl (n,H,W) -> (n,9,H,W): out[n,t,y,x] = dl[n, y - ky + 1, x - kx + 1], zero outside, t = 3 ky + kx: slices of the
    zero-padded map."""
    n, H, W = dl.shape
    p = F.pad(dl, (1, 1, 1, 1))
    return torch.stack([p[:, 2 - t // 3:2 - t // 3 + H, 2 - t % 3:2 - t % 3 + W] for t in range(9)], 1)


def add_plane(x, v, scale):
    """k_add_plane.  x (planes,HW), v (planes,) -> x + v * scale on every pixel: with scale = 1 / HW, x plus the gradient of the plane
    mean under the upstream gradient v."""
    return x + (v * scale)[:, None]


def cab_backward_reduce(dout, s):
    """k_cab_bwd_reduce.  dout, s (planes,HW).  For out = s * sig + d with one sig and one d per plane: (d out / d sig, d out / d d)
    under dout, i.e. (sum dout * s, sum dout)."""
    with torch.enable_grad():
        sig = torch.ones(s.shape[0], dtype=s.dtype, device=s.device, requires_grad=True)
        d = torch.zeros(s.shape[0], dtype=s.dtype, device=s.device, requires_grad=True)
        return _grad(s * sig[:, None] + d[:, None], [sig, d], dout)


def cab_backward_shallow(dout, gate, dsp):
    """k_cab_bwd_shallow.  dout (planes,HW), gate, dsp (planes,).  The gradient into the shallower map: through s * sigmoid(gate) under
    dout, and through its pool (mean) under dsp."""
    with torch.enable_grad():
        s = torch.zeros_like(dout).requires_grad_()
        return _grad([s * torch.sigmoid(gate)[:, None], s.mean(1)], [s], [dout, dsp])[0]


def cab_gate_preact(sp, dp, W1, b1):
    """Pre-activations of the gate's hidden layer, (n,oc); W1 (oc,2oc) in the conv layout."""
    return torch.matmul(torch.cat((sp, dp), 1), W1.t()) + b1


def cab_gate_backward(sp, dp, gate, a, badd, W1, b1, W2):
    """k_cab_gate_bwd.  g = W2 relu(W1 [sp; dp] + b1) + b2 with W1 (oc,2oc), W2 (oc,oc) in the conv layout [out][in], under the upstream
    gradient a * sigmoid'(gate) (a = d loss / d sigmoid(g); gate = the forward's g).  Returns (dW1, db1, dW2, db2, dsp, ddp), ddp plus
    badd when given (the broadcast term of the deepest CAB)."""
    with torch.enable_grad():
        sp, dp, W1, b1, W2 = [t.detach().clone().requires_grad_() for t in (sp, dp, W1, b1, W2)]
        b2 = torch.zeros(W2.shape[0], dtype=W2.dtype, device=W2.device, requires_grad=True)
        g = torch.matmul(F.relu(cab_gate_preact(sp, dp, W1, b1)), W2.t()) + b2
        sg = torch.sigmoid(gate)
        dW1, db1, dW2, db2, dsp, ddp = _grad(g, [W1, b1, W2, b2, sp, dp], a * sg * (1 - sg))
    return dW1, db1, dW2, db2, dsp, ddp if badd is None else ddp + badd
