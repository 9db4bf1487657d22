"""CPU side of tests/test_train_kernels_gpu.py: the definitions of tests/_train_refs.py are pinned here in float64 to PyTorch's own operators, so
that a wrong definition cannot pass as a right kernel, and the inputs of the GPU module are shown to tell a wrong kernel from a right one.

(a) conv_wgrad equals torch.nn.grad.conv2d_weight and dy.sum, conv_dgrad equals torch.nn.grad.conv2d_input (with rows and residual), at every
    shape of the GPU module, to 1e-12 of max|ref|.
(b) bn_stats, bn_apply_relu and bn_relu_backward equal nn.BatchNorm2d + relu under autograd, train and eval, momentum 0.1 and None (two steps, so
    that the 1 / n factor is 1 and then 1 / 2), at every size with cnt > 1; at cnt = 1, which nn.BatchNorm2d refuses, the written rule is checked
    by hand.  adam_step equals torch.optim.Adam over three steps with weight decay and AMSGrad on and off; the two loss definitions agree where
    no clamp binds.
(c) wgrad_plan gives the split plans that the GPU module's docstring names for its shapes.
(d) Mutants.  Each differs from the true reference by more than 1e-3 max|ref| at every GPU shape where it is a different function at all:
      taps transposed (dy <-> dx)                 k = 3 and more than one pixel
      the border replicated instead of zero       k = 3
      a pixel stage that ignores the sample boundary (the batch read as one map of B H rows)      k = 3, B > 1
      the bias column dropped                     every shape
      biased instead of unbiased running variance cnt <= 771 at the factor 1 / n = 1 of a first step (the two differ by f var / (cnt - 1): at
                                                  cnt = 25680 that is below the gate's own floor, and no input could show it); without the
                                                  cnt = 1 branch the unbiased rule gives 0 / 0
      the ReLU mask taken from x instead of out   every size with cnt > 1
      batch statistics used in eval mode          every size with cnt > 1
"""
import pytest
import torch
import torch.nn.functional as F

import _train_refs as T

D = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _dd(d):
    return {k: v.double() for k, v in d.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) convolution gradients
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', T.WGRAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conv_wgrad_equals_torch(shape):
    Cout, Cin, k, B, H, W = shape
    x, dy = [t.double() for t in T.wgrad_inputs(*shape)]
    dw, db = T.conv_wgrad(x, dy, k)
    assert dw.shape == (Cout, Cin, k, k) and db.shape == (Cout,)
    assert _rel(dw, torch.nn.grad.conv2d_weight(x, (Cout, Cin, k, k), dy, padding=k // 2)) < 1e-12
    assert _rel(db, dy.sum((0, 2, 3))) < 1e-12


@pytest.mark.parametrize('H,W', T.DGRAD_MAPS)
@pytest.mark.parametrize('cin,cout,k,rows', T.DGRAD_CONVS)
def test_conv_dgrad_equals_torch(cin, cout, k, rows, H, W):
    dy, w, res = [t.double() for t in T.dgrad_inputs(cin, cout, k, 2, H, W, rows)]
    ref = torch.nn.grad.conv2d_input((2, cin, H, W), w, dy, padding=k // 2)[:, :rows]
    assert _rel(T.conv_dgrad(dy, w, rows=rows), ref) < 1e-12
    assert _rel(T.conv_dgrad(dy, w, rows=rows, residual=res), ref + res) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) BatchNorm, Adam, loss
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,C,HW', [s for s in T.BN_SIZES if s[0] * s[2] > 1])
@pytest.mark.parametrize('momentum,train', [(0.1, True), (None, True), (0.1, False)])
def test_batchnorm_equals_torch(N, C, HW, momentum, train):
    d = _dd(T.bn_inputs(N, C, HW))
    bn = torch.nn.BatchNorm2d(C, eps=T.BN_EPS, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(d['gamma']), bn.bias.copy_(d['beta']), bn.running_mean.copy_(d['rmean']), bn.running_var.copy_(d['rvar'])
    bn.train(train)
    rm, rv = d['rmean'], d['rvar']
    for step in (1, 2):
        x = (d['x'] * step).requires_grad_()
        with torch.enable_grad():
            y = F.relu(bn(x.view(N, C, HW, 1)))
            y.backward(d['dy'].view(N, C, HW, 1))
        factor = (1.0 / step if momentum is None else momentum) if train else 0.0
        mean, invstd, rm, rv = T.bn_stats(x.detach(), rm, rv, T.BN_EPS, factor, train)
        out = T.bn_apply_relu(x.detach(), mean, invstd, d['gamma'], d['beta'])
        dx, dg, db = T.bn_relu_backward(d['dy'], out, x.detach(), mean, invstd, d['gamma'], train)
        assert _rel(out, y.detach().view(N, C, HW)) < 1e-12
        # the constant plane's dx is analytically 0 and torch's is rounding noise of size invstd = 316: compared on the scale of the tensor
        assert _rel(dx, x.grad) < 1e-9 and _rel(dg, bn.weight.grad) < 1e-9 and _rel(db, bn.bias.grad) < 1e-12
        assert _rel(rm, bn.running_mean) < 1e-12 and _rel(rv, bn.running_var) < 1e-12
        bn.weight.grad = bn.bias.grad = None
    assert int(bn.num_batches_tracked) == (2 if train else 0)


def test_batchnorm_single_value_rule():
    """cnt = 1: variance 0, invstd = 1 / sqrt(eps), the running variance moves towards 0 (the rule `else var`), dx = 0."""
    d = _dd(T.bn_inputs(1, 256, 1))
    mean, invstd, rm, rv = T.bn_stats(d['x'], d['rmean'], d['rvar'], T.BN_EPS, 0.25, True)
    assert torch.equal(mean, d['x'][0, :, 0]) and torch.equal(invstd, torch.full((256,), T.BN_EPS, dtype=D).rsqrt())
    assert _rel(rv, 0.75 * d['rvar']) < 1e-15 and _rel(rm, 0.75 * d['rmean'] + 0.25 * mean) < 1e-15
    out = T.bn_apply_relu(d['x'], mean, invstd, d['gamma'], d['beta'])
    assert torch.equal(out[0, :, 0], d['beta'].clamp_min(0))
    dx, dg, db = T.bn_relu_backward(d['dy'], out, d['x'], mean, invstd, d['gamma'], True)
    assert float(dx.abs().max()) == 0 and float(dg.abs().max()) == 0
    same = T.bn_stats(d['x'], d['rmean'], d['rvar'], T.BN_EPS, 0.0, True)
    assert same[2] is d['rmean'] and same[3] is d['rvar'] and T.bn_stats(d['x'], None, None, T.BN_EPS, 0.1, True)[2:] == (None, None)


@pytest.mark.parametrize('amsgrad', [True, False])
@pytest.mark.parametrize('wd', [0.0, 1e-2])
def test_adam_step_equals_torch(amsgrad, wd):
    g = T.gen(5, amsgrad, wd * 100)
    p0 = torch.randn(4100, generator=g, dtype=D)
    grads = [torch.randn(4100, generator=g, dtype=D) * s for s in (1.0, 0.1, 3.0)]      # the second step's v falls below vmax
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([param], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, amsgrad=amsgrad)
    p, m, v, vmax = p0, torch.zeros_like(p0), torch.zeros_like(p0), torch.zeros_like(p0)
    for step, gr in enumerate(grads, 1):
        param.grad = gr.clone()
        opt.step()
        p, m, v, vmax = T.adam_step(p, gr, m, v, vmax, step, 1e-3, 0.9, 0.999, 1e-8, wd, amsgrad)
        st = opt.state[param]
        assert _rel(p, param.detach()) < 1e-12 and _rel(m, st['exp_avg']) < 1e-12 and _rel(v, st['exp_avg_sq']) < 1e-12
        if amsgrad:
            assert _rel(vmax, st['max_exp_avg_sq']) < 1e-12
    assert bool((vmax > v).any()) == amsgrad


def test_loss_definitions_agree_where_no_clamp_binds():
    g = T.gen(6)
    z = (torch.randn(5, 7, generator=g, dtype=D) * 4).clamp(-15, 15)
    t = (torch.rand(5, 7, generator=g) < 0.3).double()
    a, b = T.bce(z, t, 'sigmoid'), T.bce(z, t, 'with_logits')
    assert abs(float(a - b)) < 1e-9 * float(b)
    assert float(T.bce(torch.tensor([150.0], dtype=D), torch.tensor([0.0], dtype=D), 'sigmoid')) == 100.0


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) split plans
# ---------------------------------------------------------------------------------------------------------------------------------
def _plan(Cout, Cin, k, B, H, W):
    K = B * H * W
    nsplit, kchunk = T.wgrad_plan(Cout, Cin * k * k + 1, K)
    return nsplit, kchunk, K - (nsplit - 1) * kchunk


def test_wgrad_plans():
    assert _plan(65, 64, 1, 2, 9, 15) == (3, 96, 78)
    assert _plan(129, 65, 3, 3, 7, 11) == (2, 128, 103)
    assert _plan(1, 1, 1, 2, 37, 45) == (27, 128, 2)
    assert _plan(9, 32, 1, 2, 24, 43) == (17, 128, 16)
    assert _plan(4096, 228, 3, 1, 16, 16) == (1, 256, 256) and -(-2053 // 64) * (4096 // 64) == 2112 > 2048
    assert _plan(64, 64, 3, 1, 16, 16) == (2, 128, 128) and 64 * 9 == 9 * 64
    for s in T.WGRAD_SHAPES[:6]:
        assert _plan(*s)[0] == 1
    assert _plan(63, 63, 1, 1, 8, 16)[2] == 128 == _plan(64, 7, 3, 1, 8, 16)[2] and 63 + 1 == 64 == 7 * 9 + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) mutants
# ---------------------------------------------------------------------------------------------------------------------------------
SEP = 1e-3


def _apart(mutant, ref):
    return float((mutant - ref).abs().max()) > SEP * float(ref.abs().max())


def _wgrad_replicated(x, dy, k):
    B, Cin, H, W = x.shape
    cols = F.unfold(F.pad(x, (1, 1, 1, 1), mode='replicate'), k).permute(1, 0, 2).reshape(Cin * k * k, B * H * W)
    rows = dy.reshape(B, dy.shape[1], H * W).permute(1, 0, 2).reshape(dy.shape[1], B * H * W)
    return (rows @ cols.t()).reshape(dy.shape[1], Cin, k, k)


@pytest.mark.parametrize('shape', T.WGRAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_wgrad_mutants_are_told_apart(shape):
    Cout, Cin, k, B, H, W = shape
    x, dy = [t.double() for t in T.wgrad_inputs(*shape)]
    dw, db = T.conv_wgrad(x, dy, k)
    assert _apart(torch.zeros_like(db), db)                                          # the bias column dropped
    if k == 3:
        assert _apart(_wgrad_replicated(x, dy, k), dw)                               # border replicated
        if H * W > 1:
            assert _apart(dw.transpose(2, 3), dw)                                    # taps transposed
        if B > 1:                                                                    # the rows of the next sample read as neighbours
            one = T.conv_wgrad(x.transpose(0, 1).reshape(1, Cin, B * H, W), dy.transpose(0, 1).reshape(1, Cout, B * H, W), k)[0]
            assert _apart(one, dw)
    assert sum(s[2] == 3 and s[3] > 1 for s in T.WGRAD_SHAPES) >= 2


@pytest.mark.parametrize('N,C,HW', T.BN_SIZES)
def test_batchnorm_mutants_are_told_apart(N, C, HW):
    d = _dd(T.bn_inputs(N, C, HW))
    cnt = N * HW
    mean, invstd, rm, rv = T.bn_stats(d['x'], d['rmean'], d['rvar'], T.BN_EPS, 1.0, True)
    var = ((d['x'] - mean[None, :, None]) ** 2).mean(dim=(0, 2))
    if 1 < cnt <= 771:
        assert _apart(var, rv)                               # biased running variance
    if cnt == 1:
        assert not bool(torch.isfinite(var * cnt / (cnt - 1.0)).any()) and bool(torch.isfinite(rv).all())
    out = T.bn_apply_relu(d['x'], mean, invstd, d['gamma'], d['beta'])
    dead = float((out == 0).double().mean())
    if cnt * C >= 255:
        assert 0.3 < dead < 0.7, dead
    for train in (True, False):
        dx = T.bn_relu_backward(d['dy'], out, d['x'], mean, invstd, d['gamma'], train)[0]
        from_x = T.bn_relu_backward(d['dy'], d['x'], d['x'], mean, invstd, d['gamma'], train)[0]          # the mask from x
        if cnt > 1:
            assert bool(((out > 0) != (d['x'] > 0)).any()) and _apart(from_x, dx)
    e_mean, e_invstd = T.bn_stats(d['x'], d['rmean'], d['rvar'], T.BN_EPS, 0.0, False)[:2]
    if cnt > 1:                                                                      # batch statistics in eval mode
        assert _apart(mean, e_mean) and _apart(invstd, e_invstd)
        assert _apart(out, T.bn_apply_relu(d['x'], e_mean, e_invstd, d['gamma'], d['beta']))
    if C > 3 and cnt >= 255:                                                         # the kernel's one-pass fp64 variance on the offset plane
        xo = d['x'][:, T.BN_OFFSET]
        one_pass = (xo * xo).sum() / cnt - (xo.sum() / cnt) ** 2
        # q / cnt and m^2 are each rounded to 2^-53 of about 1e4 and a few more such roundings sit in the sums: 4 x 2^-53 x mean^2, which is
        # 4.4e-8 of a variance of 1e-4 and moves invstd by half of that, far inside the gate's 1e-6
        assert abs(float(one_pass - var[T.BN_OFFSET])) <= 4 * 2.0 ** -53 * float(xo.mean()) ** 2 < 1e-7 * float(var[T.BN_OFFSET])
    if C > 3:
        assert float(out[:, T.BN_DEAD].abs().max()) == 0 and float(var[T.BN_CONST]) == 0 and (cnt == 1 or 0 < float(var[T.BN_OFFSET]) < 1e-3)
