"""Plain torch definitions of the kernels of the refiner's training step that sum (csrc/refiner_train.hip: the weight gradient and its slab
reduce, the five BatchNorm kernels; the input gradient as model/refiner_train.py builds it from flipped weights) and of csrc/train_step.hip
(loss tail, Adam / AMSGrad, the device-scalar scale), with the shapes and seeded inputs that tests/test_train_kernels_gpu.py runs them at.

No project code.  Every function works in the dtype and on the device of its arguments, so the same text serves as the float64 reference on
the CPU and as the fp32 yardstick on the GPU.  The convolution gradients are F.unfold plus one matrix product (no torch.nn.grad call, hence no
MIOpen kernel search on the GPU).  tests/test_train_refs.py pins every definition to PyTorch's own operators in float64 and shows that the
inputs below tell a wrong kernel from a right one.
"""
import torch
import torch.nn.functional as F


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# convolution gradients (stride 1, pad k // 2, k = 1 or 3)
# ---------------------------------------------------------------------------------------------------------------------------------
def conv_wgrad(x, dy, k):
    """x (B,Cin,H,W), dy (B,Cout,H,W) -> (dW (Cout,Cin,k,k), dbias (Cout)):  dW[co,ci,ky,kx] = sum_{n,y,x} dy[n,co,y,x] x[n,ci,y+ky-p,x+kx-p],
    zero outside the map."""
    B, Cin, H, W = x.shape
    Cout = dy.shape[1]
    cols = F.unfold(x, k, padding=k // 2).permute(1, 0, 2).reshape(Cin * k * k, B * H * W)       # [ci * k k + t][pixel]
    rows = dy.reshape(B, Cout, H * W).permute(1, 0, 2).reshape(Cout, B * H * W)
    return (rows @ cols.t()).reshape(Cout, Cin, k, k), dy.sum(dim=(0, 2, 3))


def conv_dgrad(dy, w, rows=None, residual=None):
    """dy (B,Cout,H,W), w (Cout,Cin,k,k) -> dx (B,Cin,H,W) (+ residual): dx[n,ci,y,x] = sum_{co,ky,kx} w[co,ci,ky,kx] dy[n,co,y-ky+p,x-kx+p], a
    forward conv of dy with the flipped, transposed weights.  ``rows``: only the first input channels."""
    B, Cout, H, W = dy.shape
    k = w.shape[2]
    wt = w.flip(2, 3).transpose(0, 1)                             # [ci][co][a][b] = w[co][ci][k-1-a][k-1-b]
    if rows is not None:
        wt = wt[:rows]
    cols = F.unfold(dy, k, padding=k // 2)                        # (B, Cout k k, HW)
    dx = (wt.reshape(wt.shape[0], Cout * k * k) @ cols).reshape(B, wt.shape[0], H, W)
    return dx if residual is None else dx + residual


def wgrad_plan(Cout, ncol, K):
    """(nsplit, kchunk) of csrc/refiner_train.hip: wgrad_plan, in integers: 64 x 64 tiles of (co, column), at most 2048 / tiles splits, each of at
    least one 128-pixel chain, the chunk rounded up to whole 32-pixel stages."""
    tiles = -(-ncol // 64) * -(-Cout // 64)
    most = -(-K // 128)
    s = min(max(2048 // tiles, 1), most)
    c = -(-K // s)
    c = -(-c // 32) * 32
    return -(-K // c), c


# (Cout, Cin, k, B, H, W); what each reaches: the module docstring of tests/test_train_kernels_gpu.py
WGRAD_SHAPES = [(1, 1, 1, 1, 1, 1), (1, 1, 3, 1, 1, 1), (3, 2, 3, 1, 1, 33), (5, 7, 3, 2, 5, 1), (63, 63, 1, 1, 8, 16), (64, 7, 3, 1, 8, 16),
                (65, 64, 1, 2, 9, 15), (129, 65, 3, 3, 7, 11), (64, 64, 3, 1, 16, 16), (1, 1, 1, 2, 37, 45), (9, 32, 1, 2, 24, 43),
                (4096, 228, 3, 1, 16, 16)]


def wgrad_inputs(Cout, Cin, k, B, H, W):
    """(x, dy), fp32: independent normal draws, so neither the maps nor the taps are symmetric."""
    g = gen(Cout, Cin, k, B, H, W, 1)
    return torch.randn(B, Cin, H, W, generator=g), torch.randn(B, Cout, H, W, generator=g)


# (cin, cout, k, rows) and the maps of the input-gradient checks
DGRAD_CONVS = [(65, 65, 3, None), (65, 65, 3, 64), (64, 32, 3, None), (64, 64, 1, None), (32, 1, 3, None)]
DGRAD_MAPS = [(1, 1), (1, 7), (5, 1), (37, 53)]


def dgrad_inputs(cin, cout, k, B, H, W, rows):
    """(dy, w, residual), fp32; the weights scaled by 1 / sqrt(fan-in) as an initialised conv's are."""
    g = gen(cin, cout, k, B, H, W, 2)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    dy = torch.randn(B, cout, H, W, generator=g)
    return dy, w, torch.randn(B, rows or cin, H, W, generator=g)


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU.  x (N,C,HW); per-channel vectors (C)
# ---------------------------------------------------------------------------------------------------------------------------------
def _c(v):
    return v[None, :, None]


def bn_stats(x, rmean, rvar, eps, factor, train):
    """(mean, invstd, new rmean, new rvar).  train: the batch mean and the biased variance over cnt = N HW normalise; the running statistics move
    by r = (1 - f) r + f stat with the unbiased variance, var cnt / (cnt - 1) if cnt > 1 else var (nn.BatchNorm2d refuses cnt = 1; the kernel
    documents this rule), and stay as they are when they are None or f = 0.  eval: mean and invstd from the running statistics."""
    if not train:
        return rmean, 1.0 / torch.sqrt(rvar + eps), rmean, rvar
    cnt = x.shape[0] * x.shape[2]
    mean = x.mean(dim=(0, 2))
    var = ((x - _c(mean)) ** 2).mean(dim=(0, 2))
    invstd = 1.0 / torch.sqrt(var + eps)
    if rmean is None or factor == 0:
        return mean, invstd, rmean, rvar
    unbiased = var * cnt / (cnt - 1) if cnt > 1 else var
    return mean, invstd, (1 - factor) * rmean + factor * mean, (1 - factor) * rvar + factor * unbiased


def bn_apply_relu(x, mean, invstd, gamma, beta):
    return torch.relu((x - _c(mean)) * _c(invstd * gamma) + _c(beta))


def bn_relu_backward(dy, out, x, mean, invstd, gamma, train):
    """(dx, dgamma, dbeta) of relu(batch_norm(x)) from the saved output: g = dy where out > 0, else 0.  xhat is centred on the mean that is handed
    in; in the last term of dx its own mean is taken out, as the kernel documents (nothing in exact arithmetic, where that mean is 0)."""
    g = torch.where(out > 0, dy, torch.zeros_like(dy))
    xhat = (x - _c(mean)) * _c(invstd)
    dbeta, dgamma = g.sum(dim=(0, 2)), (g * xhat).sum(dim=(0, 2))
    if not train:
        return _c(gamma * invstd) * g, dgamma, dbeta
    cnt = x.shape[0] * x.shape[2]
    return _c(gamma * invstd) * (g - _c(dbeta) / cnt - (xhat - _c(xhat.mean(dim=(0, 2)))) * _c(dgamma) / cnt), dgamma, dbeta


# (N, C, HW); what each reaches: the module docstring of tests/test_train_kernels_gpu.py
BN_SIZES = [(1, 1, 1), (3, 1, 1), (1, 1, 255), (3, 64, 257), (1, 64, 25680), (3, 256, 255), (1, 257, 257), (3, 257, 1), (1, 256, 1)]
BN_EPS = 1e-5
BN_OFFSET, BN_CONST, BN_DEAD = 1, 2, 3                            # the channels with special data, where C > 3


def bn_inputs(N, C, HW):
    """dict of fp32 tensors x, dy (N,C,HW), gamma, beta, rmean, rvar (C).  Ordinary channels: x = 0.3 + 2 randn, small beta, so about half the
    pixels are dead after the ReLU and sign(x) is not the mask.  Where C > 3: channel 1 is an offset plane (100 + 0.01 randn), channel 2 a constant
    plane (3.0: every sum is exact, the variance is 0), channel 3 has beta = -50, which no normalised value times gamma <= 1.5 reaches: out = 0."""
    g = gen(N, C, HW, 3)
    x = torch.randn(N, C, HW, generator=g) * 2 + 0.3
    d = dict(dy=torch.randn(N, C, HW, generator=g), gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g) * 0.1,
             rmean=torch.randn(C, generator=g) * 0.1, rvar=torch.rand(C, generator=g) + 0.5)
    if C > 3:
        x[:, BN_OFFSET] = 100 + 0.01 * torch.randn(N, HW, generator=g)
        x[:, BN_CONST] = 3.0
        d['beta'][BN_DEAD] = -50.0
    d['x'] = x
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# loss tail, Adam, scale
# ---------------------------------------------------------------------------------------------------------------------------------
def bce(z, t, definition):
    """Mean binary cross-entropy of logits z against targets t: 'sigmoid' = BCELoss(sigmoid(z)) (its logs clamped at -100), 'with_logits' the
    softplus form.  As functions of real numbers the two agree wherever the clamp does not bind."""
    if definition == 'sigmoid':
        return F.binary_cross_entropy(torch.sigmoid(z), t)
    assert definition == 'with_logits'
    return F.binary_cross_entropy_with_logits(z, t)


def adam_step(p, g, m, v, vmax, step, lr, beta1, beta2, eps, weight_decay, amsgrad):
    """torch.optim.Adam's single-tensor update, written out: (p, m, v, vmax) after step number ``step`` (1-based); vmax passes through without
    AMSGrad.  Weight decay is folded into the gradient."""
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (g - m) * (1 - beta1)
    v = beta2 * v + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    if amsgrad:
        vmax = torch.maximum(vmax, v)
        denom = vmax.sqrt() / bc2 ** 0.5 + eps
    else:
        denom = v.sqrt() / bc2 ** 0.5 + eps
    return p - (lr / bc1) * (m / denom), m, v, vmax


def scale_by(x, s):
    return x * s
