"""Training pass of the refinement network on the HIP kernels: ``SegNetwork.forward_train`` (model/seg_network.py).

One ``torch.autograd.Function`` covers the whole network.  Its forward runs the inference kernels (frtm_conv2d, csrc/refiner_ops.hip)
with the weights packed per call (they change every optimiser step), BatchNorm through frtm_bn_stats / frtm_bn_apply_relu (batch
statistics and the running-statistics update in train mode, running statistics in eval mode), and keeps what the backward needs.
Its backward (csrc/refiner_train.hip) gives the gradient of every parameter that requires one:
  * weight / bias gradients: frtm_conv_wgrad (fp32 MFMA over pixel chunks, fixed-order fp64 sum of the chunks);
  * input gradients: frtm_conv2d on the flipped, transposed weights (3x3) or the transposed weights (1x1), residual sums in its epilogue;
  * ReLU, BatchNorm, bicubic 2x, bilinear and channel-attention transposes: one kernel each, gather form;
  * head tail: conv2's nine taps are shifted first (frtm_shift9), then the nine maps go through the two resampling transposes, so the
    32-channel full-resolution tensor of the head is neither formed nor kept (the identity of frtm_tap_mix).
No sum uses atomics, so two identical backward passes give bitwise identical gradients.  No gradient flows into the scores or the
backbone taps (the input gradient of TSE.reduce[0] is not computed).

Under ``SegNetwork.train_precision = 'bf16x1'`` the 3x3 forward and input-gradient convs that ops.bf16x1_3x3_launch routes and the 3x3 weight
gradients that ops.bf16x1_wgrad_launch routes run on the bf16 form (operands rounded once to bf16, bf16 MFMAs, fp32 accumulation); everything
else -- 1x1 convs and their gradients, BatchNorm, the glue kernels, the head's tap-map weight gradient, what is saved -- stays fp32.
"""
import torch
from torch import nn

from .. import _hip as H
from .. import ops
from .seg_network import BackwardCompatibleUpsampler, Upsampler, cab_level, project_head


def _flipT(w):
    """Input-gradient weights of a stride-1, pad-k//2 conv: (Cout,Cin,k,k) -> (Cin,Cout,k,k), taps reversed."""
    return w.detach().flip(2, 3).transpose(0, 1).contiguous()


class _Runner:
    """Per-call conv launcher: packs each weight into the layout its launch needs."""

    def __init__(self, net, dev):
        self.net, self.dev = net, dev
        self.bf16 = net.train_precision == 'bf16x1'
        self._ones = {}

    def ones(self, c):
        if c not in self._ones:
            self._ones[c] = H.fill(torch.empty(c, device=self.dev), 1.0)
        return self._ones[c]

    def conv(self, x, w, bias=None, relu=False, residual=None):
        w = w.detach()
        cout, k = w.shape[0], w.shape[2]
        shift = None if bias is None else bias.detach().float().contiguous()
        scale = None if shift is None else self.ones(cout)
        n, cin, hh, ww = x.shape
        if k == 3 and self.bf16 and ops.bf16x1_3x3_launch(n, hh, ww, cin, cout, self.net.bf16_min_blocks):
            wB = ops.pack_weights(w, bf16x1=True)[0]
            return ops.conv2d(x, wB, cout, 3, 1, 1, scale=scale, shift=shift, residual=residual, relu=relu, splitk=1, w_layout=7)
        if k == 3 and self.net.use_winograd and ops.wino_launch(n, hh, ww, cout):
            wW = ops.pack_weights(w, wino=True)[0]
            return ops.conv2d(x, wW, cout, 3, 1, 1, scale=scale, shift=shift, residual=residual, relu=relu, splitk=1, w_layout=2)
        wT, ktab, lay = ops.pack_weights(w)
        return ops.conv2d(x, wT, cout, k, 1, k // 2, ktab=ktab, scale=scale, shift=shift, residual=residual, relu=relu, w_layout=lay)

    def dgrad(self, dy, w, residual=None, rows=None):
        """Input gradient of a stride-1 conv; ``rows``: only the first input channels.  A forward conv of the transposed channel pair: conv's
        routing rules see (Cout, Cin or rows)."""
        wt = _flipT(w) if w.shape[2] == 3 else w.detach().transpose(0, 1).contiguous()
        if rows is not None:
            wt = wt[:rows].contiguous()
        return self.conv(dy, wt, residual=residual)


def _bn_factor(bn):
    if not (bn.training and bn.track_running_stats):
        return 0.0
    bn.num_batches_tracked.add_(1)
    return 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else float(bn.momentum)


def _rrb_forward(R, m, x):
    a = R.conv(x, m.conv1x1.weight, m.conv1x1.bias)
    first, last = m.bblock[0], m.bblock[-1]
    s = dict(x=x, a=a)
    if isinstance(m.bblock[1], nn.BatchNorm2d):
        bn = m.bblock[1]
        bpre = R.conv(a, first.weight, first.bias)
        batch = bn.training or bn.running_mean is None
        factor = _bn_factor(bn) if batch else 0.0
        mean, invstd = ops.bn_stats(bpre, bn.running_mean, bn.running_var, bn.eps, factor, batch)
        e = ops.bn_apply_relu(bpre, mean, invstd, bn.weight.detach().contiguous(), bn.bias.detach().contiguous())
        s.update(bpre=bpre, mean=mean, invstd=invstd, batch=batch)
    else:
        e = R.conv(a, first.weight, first.bias, relu=True)
    out = R.conv(e, last.weight, None, relu=True, residual=a)
    s.update(e=e, out=out)
    return out, s


def _cab_weights(cab):
    """The gate's two 1x1 convs as ops.cab_gate takes them: the weights transposed to [in][out]."""
    c = cab.convreluconv
    return (c[0].weight.detach().flatten(1).t().contiguous(), c[0].bias.detach(), c[2].weight.detach().flatten(1).t().contiguous(),
            c[2].bias.detach())


class _Grads:
    """Collects parameter gradients by identity; ``want(p)``: whether p needs one."""

    def __init__(self, params, needs, net=None):
        self.bf16 = net is not None and net.train_precision == 'bf16x1'
        self.min_blocks = None if net is None else net.bf16_min_blocks
        self.index = {id(p): i for i, p in enumerate(params)}
        self.needs = needs
        self.out = [None] * len(params)

    def want(self, p):
        return p is not None and self.needs[self.index[id(p)]]

    def put(self, p, g):
        if g is not None and self.want(p):
            self.out[self.index[id(p)]] = g.view(p.shape)

    def conv(self, m, dy, x, w=None):
        """weight / bias gradients of conv module m (skipped when frozen)."""
        ww, wb = self.want(m.weight), self.want(m.bias)
        if ww or wb:
            k = m.weight.shape[2]
            n, cout, hh, wd = dy.shape
            bf = k == 3 and self.bf16 and ops.bf16x1_wgrad_launch(n, hh, wd, x.shape[1], cout, self.min_blocks)
            dw, db = ops.conv_wgrad(dy, x, k, weight=ww, bias=wb, bf16x1=bf)
            self.put(m.weight, dw)
            self.put(m.bias, db)


def _rrb_backward(R, G, m, s, dout):
    first, last = m.bblock[0], m.bblock[-1]
    gout = ops.relu_backward(dout, s['out'])
    G.conv(last, gout, s['e'])
    de = R.dgrad(gout, last.weight)
    if 'bpre' in s:
        bn = m.bblock[1]
        affine = G.want(bn.weight) or G.want(bn.bias)
        gb, dgam, dbet = ops.bn_relu_backward(de, s['e'], s['bpre'], s['mean'], s['invstd'], bn.weight.detach().contiguous(), s['batch'],
                                              affine=affine)
        G.put(bn.weight, dgam)
        G.put(bn.bias, dbet)
    else:
        gb = ops.relu_backward(de, s['e'], out=de)
    G.conv(first, gb, s['a'])
    da = R.dgrad(gb, first.weight, residual=gout)
    G.conv(m.conv1x1, da, s['x'])
    return R.dgrad(da, m.conv1x1.weight)


class _RefinerTrain(torch.autograd.Function):

    @staticmethod
    def forward(ctx, net, scores, image_size, n_feat, *args):
        feats, params = args[:n_feat], args[n_feat:]
        levels = list(net.ft_channels)
        dev = scores.device
        R = _Runner(net, dev)
        scores = scores.detach().float().contiguous()
        sv = {}
        for L, ft in zip(levels, feats):
            T = net.TSE[L]
            ft = ft.detach().float().contiguous()
            r0 = R.conv(ft, T.reduce[0].weight, T.reduce[0].bias, relu=True)
            h = R.conv(r0, T.reduce[2].weight, T.reduce[2].bias)
            s = scores if tuple(scores.shape[-2:]) == tuple(h.shape[-2:]) else ops.bilinear_resize(scores, h.shape[-2:])
            x65 = torch.cat((h, s), dim=1)
            t0 = R.conv(x65, T.transform[0].weight, T.transform[0].bias, relu=True)
            t2 = R.conv(t0, T.transform[2].weight, T.transform[2].bias, relu=True)
            t4 = R.conv(t2, T.transform[4].weight, T.transform[4].bias, relu=True)
            r, rs1 = _rrb_forward(R, net.RRB1[L], t4)
            sv[L] = dict(ft=ft, h=h, r0=r0, x65=x65, t0=t0, t2=t2, t4=t4, rrb1=rs1, r=r, hw=tuple(h.shape[-2:]))
        x, pool0 = None, ops.plane_mean(sv[levels[0]].pop('h'))
        for L in levels:
            v = sv[L]
            sp = ops.plane_mean(v['r'])
            out, gate, dp = cab_level(v['r'], sp, x, pool0, _cab_weights(net.CAB[L]), 0)       # one object per frame: nothing shared
            v.update(sp=sp, dp=dp, gate=gate, deeper_hw=(1, 1) if x is None else tuple(x.shape[-2:]))
            x, v['rrb2'] = _rrb_forward(R, net.RRB2[L], out)
        pj = net.project
        u1 = ops.pyrup2x(x)
        y = R.conv(u1, pj.conv1.weight, pj.conv1.bias, relu=True)
        # always fused and on conv2's nine tap maps where the resize fits: the backward rests on the tap-mix identity either way
        logits = project_head(y, pj.conv2.weight.detach().contiguous(), pj.conv2.bias.detach().contiguous(), image_size, False, True, True)
        ctx.net, ctx.sv, ctx.head = net, sv, dict(u1=u1, y=y, hw=tuple(x.shape[-2:]))
        ctx.params = params
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        net, sv = ctx.net, ctx.sv
        params = ctx.params
        n_feat = len(net.ft_channels)
        G = _Grads(params, ctx.needs_input_grad[4 + n_feat:], net)
        R = _Runner(net, dlogits.device)
        levels = list(net.ft_channels)
        dl = dlogits.detach().float().contiguous()
        n, _, Ho, Wo = dl.shape
        pj = net.project
        u1, y = ctx.head['u1'], ctx.head['y']
        hh, ww = ctx.head['hw']
        # head tail: T_t = Pyr^T(Bil^T(shift_t(dl))) at (2hh, 2ww); dy_c = sum_t w2[c,t] T_t; dW2[c,t] = sum y_c T_t; db2 = sum dl
        S = ops.shift9(dl)
        if (Ho, Wo) != (4 * hh, 4 * ww):
            S = ops.bilinear_backward(S, 4 * hh, 4 * ww)
        Tm = ops.pyrup2x_backward(S)
        del S
        c2 = y.shape[1]
        ww2, wb2 = G.want(pj.conv2.weight), G.want(pj.conv2.bias)
        if ww2 or wb2:
            if ww2:
                g9, _ = ops.conv_wgrad(Tm, y, 1, bias=False)              # (9, c2): tap x channel
                G.put(pj.conv2.weight, g9.view(9, c2).t().contiguous())
            if wb2:
                G.put(pj.conv2.bias, ops.conv_wgrad(dl, dl, 1, weight=False)[1])     # sum of dl (the bias column of a 1 x 1 problem)
        dy = R.conv(Tm, pj.conv2.weight.detach().view(c2, 9, 1, 1))
        del Tm
        gy = ops.relu_backward(dy, y, out=dy)
        G.conv(pj.conv1, gy, u1)
        dx = ops.pyrup2x_backward(R.dgrad(gy, pj.conv1.weight))
        dpool0 = None
        for i in reversed(range(len(levels))):
            L = levels[i]
            v = sv[L]
            dout = _rrb_backward(R, G, net.RRB2[L], v['rrb2'], dx)
            r, gate = v['r'], v['gate']
            a, b = ops.cab_backward_reduce(dout, r)
            cr = net.CAB[L].convreluconv
            cp = (cr[0].weight, cr[0].bias, cr[2].weight, cr[2].bias)
            *gw, dsp, ddp = ops.cab_gate_backward(v['sp'], v['dp'], gate, a, b if i == 0 else None, cr[0].weight.detach(), cr[0].bias.detach(),
                                                  cr[2].weight.detach(), grads=[G.want(p) for p in cp])
            for p, g in zip(cp, gw):
                G.put(p, g)
            dr = ops.cab_backward_shallow(dout, gate, dsp)
            if i == 0:
                dpool0 = ddp                     # deepest: the deeper input is pool0 = mean(TSE.reduce(ft)) itself (gate and broadcast)
            else:
                hd, wd = v['deeper_hw']
                dx = ops.bilinear_backward(dout, hd, wd)
                ops.add_plane_(dx, ddp, 1.0 / (hd * wd))
            del dout
            dt4 = _rrb_backward(R, G, net.RRB1[L], v['rrb1'], dr)
            T = net.TSE[L]
            g4 = ops.relu_backward(dt4, v['t4'], out=dt4)
            G.conv(T.transform[4], g4, v['t2'])
            g2 = ops.relu_backward(R.dgrad(g4, T.transform[4].weight), v['t2'])
            G.conv(T.transform[2], g2, v['t0'])
            g0 = ops.relu_backward(R.dgrad(g2, T.transform[2].weight), v['t0'])
            G.conv(T.transform[0], g0, v['x65'])
            oc = T.reduce[2].weight.shape[0]
            need_r2 = G.want(T.reduce[2].weight) or G.want(T.reduce[2].bias)
            need_r0 = G.want(T.reduce[0].weight) or G.want(T.reduce[0].bias)
            if not (need_r2 or need_r0):
                continue
            dh = R.dgrad(g0, T.transform[0].weight, rows=oc)          # the feature rows only: no gradient into the score channel
            if i == 0:
                ops.add_plane_(dh, dpool0, 1.0 / (dh.shape[2] * dh.shape[3]))
            G.conv(T.reduce[2], dh, v['r0'])
            if need_r0:
                g = ops.relu_backward(R.dgrad(dh, T.reduce[2].weight), v['r0'])
                G.conv(T.reduce[0], g, v['ft'])                        # no input gradient into the backbone taps
        ctx.sv = ctx.head = None
        return (None, None, None, None) + (None,) * n_feat + tuple(G.out)


def forward_train(net, scores, features, image_size):
    """See SegNetwork.forward_train."""
    if isinstance(net.project, Upsampler):
        raise NotImplementedError('SegNetwork.forward_train: the bicubic head (Upsampler) has no HIP backward; train it through forward_torch')
    if not isinstance(net.project, BackwardCompatibleUpsampler):
        raise NotImplementedError('SegNetwork.forward_train: no HIP backward for the head %s; use forward_torch' % type(net.project).__name__)
    levels = list(net.ft_channels)
    feats = [features[L] for L in levels]
    for t in [scores] + feats:
        if not t.is_cuda:
            raise RuntimeError('SegNetwork.forward_train: tensor on %s; the HIP training path runs on the GPU only (no CPU fallback)' % t.device)
    if scores.requires_grad or any(t.requires_grad for t in feats):
        raise ValueError('SegNetwork.forward_train: scores and backbone features must not require grad (no gradient is produced for them)')
    if any(t.shape[0] != scores.shape[0] for t in feats):
        raise ValueError('SegNetwork.forward_train: one object per frame (scores %d samples, features %s frames)'
                         % (scores.shape[0], [t.shape[0] for t in feats]))
    params = list(net.parameters())
    return _RefinerTrain.apply(net, scores, tuple(int(s) for s in image_size[-2:]), len(feats), *feats, *params)
