"""SegNetwork.forward_train (model/refiner_train.py, csrc/refiner_train.hip) on the GPU: every new kernel against the fp64 definition,
the whole network's logits, parameter gradients and BatchNorm running statistics, determinism, the absence of framework compute,
frozen parameters and TrainerModel(refiner_backend='hip').

Gate (per tensor): max|g_hip - g64| <= max(4 * max|g_torch32 - g64|, 1e-6 * max|g64|), where g64 is PyTorch autograd in float64 on the
CPU (on the GPU for the B = 16 case) and g_torch32 the same op in fp32 on the GPU (MIOpen / PyTorch kernels)."""
import copy
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(autouse=True)
def _grad_mode_on():
    """These tests need autograd; other GPU test modules switch grad mode off process-wide at import or in their tests."""
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    yield
    torch.set_grad_enabled(prev)


def _err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def _gate(hip, ref64, t32, what, floor=None):
    e, e32 = _err(hip, ref64), _err(t32, ref64)
    bound = max(4 * e32, 1e-6 * float(ref64.detach().abs().max()), floor or 0.0)
    assert e <= bound, '%s: hip err %.3e, torch32 err %.3e, bound %.3e' % (what, e, e32, bound)
    return e / max(e32, 1e-30)


# ---------------------------------------------------------------------------------------------------------------------------------
# per op
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cin,cout,k,B,Hh,Ww', [(2048, 64, 1, 2, 15, 27), (256, 64, 1, 3, 31, 53), (64, 64, 1, 2, 17, 29),
                                                (65, 65, 3, 2, 23, 37), (65, 64, 3, 2, 19, 33), (64, 32, 3, 2, 41, 57),
                                                (32, 1, 3, 2, 37, 45), (32, 9, 1, 3, 240, 427)])
def test_conv_wgrad(cin, cout, k, B, Hh, Ww):
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(cin + cout + k)
    x = torch.randn(B, cin, Hh, Ww, generator=g, dtype=torch.float64)
    dy = torch.randn(B, cout, Hh, Ww, generator=g, dtype=torch.float64)
    w64 = torch.nn.grad.conv2d_weight(x, (cout, cin, k, k), dy, padding=k // 2)
    b64 = dy.sum((0, 2, 3))
    w32 = torch.nn.grad.conv2d_weight(x.float().to(DEV), (cout, cin, k, k), dy.float().to(DEV), padding=k // 2)
    b32 = dy.float().to(DEV).sum((0, 2, 3))
    dw, db = ops.conv_wgrad(dy.float().to(DEV), x.float().to(DEV), k)
    _gate(dw, w64, w32, 'dW')
    _gate(db, b64, b32, 'dbias')
    dw2, db2 = ops.conv_wgrad(dy.float().to(DEV), x.float().to(DEV), k)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


@pytest.mark.parametrize('cin,cout,k', [(65, 65, 3), (64, 32, 3), (64, 64, 1)])
def test_conv_dgrad(cin, cout, k):
    from frtm_vos_amd.model.refiner_train import _Runner
    from frtm_vos_amd.model.seg_network import SegNetwork
    g = torch.Generator().manual_seed(5)
    w = torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5
    dy = torch.randn(2, cout, 37, 53, generator=g, dtype=torch.float64)
    ref = torch.nn.grad.conv2d_input((2, cin, 37, 53), w, dy, padding=k // 2)
    t32 = torch.nn.grad.conv2d_input((2, cin, 37, 53), w.float().to(DEV), dy.float().to(DEV), padding=k // 2)
    net = SegNetwork(1, 8, {'layer4': 8}, False)
    R = _Runner(net, DEV)
    _gate(R.dgrad(dy.float().to(DEV), w.float().to(DEV)), ref, t32, 'dgrad')


@pytest.mark.parametrize('h,w', [(1, 1), (1, 3), (2, 2), (3, 1), (3, 5), (7, 11), (30, 54), (120, 214)])
def test_pyrup2x_backward(h, w):
    from frtm_vos_amd import ops
    from frtm_vos_amd.model.seg_network import PyrUpBicubic2d
    g = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(2, 3, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(2, 3, 2 * h, 2 * w, generator=g, dtype=torch.float64)
    up = PyrUpBicubic2d(3)
    up(x).backward(dout)
    x32 = x.detach().float().to(DEV).requires_grad_()
    up.to(DEV)(x32).backward(dout.float().to(DEV))
    _gate(ops.pyrup2x_backward(dout.float().to(DEV)), x.grad, x32.grad, 'pyrup bwd')


@pytest.mark.parametrize('h,w,Ho,Wo', [(15, 27, 30, 54), (30, 54, 60, 107), (60, 107, 120, 214), (480, 856, 480, 854), (1, 1, 7, 9),
                                       (1, 1, 120, 214), (20, 30, 9, 13), (3, 2, 17, 5)])
def test_bilinear_backward(h, w, Ho, Wo):
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(h + w + Ho)
    x = torch.randn(2, 2, h, w, generator=g, dtype=torch.float64, requires_grad=True)
    dout = torch.randn(2, 2, Ho, Wo, generator=g, dtype=torch.float64)
    F.interpolate(x, (Ho, Wo), mode='bilinear', align_corners=False).backward(dout)
    x32 = x.detach().float().to(DEV).requires_grad_()
    F.interpolate(x32, (Ho, Wo), mode='bilinear', align_corners=False).backward(dout.float().to(DEV))
    _gate(ops.bilinear_backward(dout.float().to(DEV), h, w), x.grad, x32.grad, 'bilinear bwd')


@pytest.mark.parametrize('momentum,train', [(0.1, True), (None, True), (0.1, False)])
def test_batchnorm_relu(momentum, train):
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(3)
    C = 64
    bn64 = torch.nn.BatchNorm2d(C, momentum=momentum).double()
    with torch.no_grad():
        bn64.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn64.bias.copy_(torch.randn(C, generator=g) * 0.1)
        bn64.running_var.copy_(torch.rand(C, generator=g) + 0.5)
        bn64.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
    bn32 = copy.deepcopy(bn64).float().to(DEV)
    rm, rv = bn32.running_mean.clone(), bn32.running_var.clone()
    nbt = 0
    bn64.train(train)
    bn32.train(train)
    for step in range(3):
        x = torch.randn(3, C, 29, 41, generator=g, dtype=torch.float64) * 2 + 0.3
        dy = torch.randn(3, C, 29, 41, generator=g, dtype=torch.float64)
        x64 = x.clone().requires_grad_()
        y64 = F.relu(bn64(x64))
        y64.backward(dy)
        x32 = x.float().to(DEV).requires_grad_()
        y32 = F.relu(bn32(x32))
        y32.backward(dy.float().to(DEV))
        xd = x.float().to(DEV)
        factor = 0.0
        if train:
            nbt += 1
            factor = 1.0 / nbt if momentum is None else momentum
        mean, invstd = ops.bn_stats(xd, rm, rv, 1e-5, factor, train)
        y = ops.bn_apply_relu(xd, mean, invstd, bn32.weight.detach(), bn32.bias.detach())
        dx, dg, db = ops.bn_relu_backward(dy.float().to(DEV), y, xd, mean, invstd, bn32.weight.detach(), train)
        _gate(y, y64, y32, 'bn out')
        _gate(dx, x64.grad, x32.grad, 'bn dx')
        _gate(dg, bn64.weight.grad, bn32.weight.grad, 'bn dgamma')
        _gate(db, bn64.bias.grad, bn32.bias.grad, 'bn dbeta')
        for p in (bn64.weight, bn64.bias, bn32.weight, bn32.bias):
            p.grad = None
        _gate(rm, bn64.running_mean, bn32.running_mean, 'running_mean')
        _gate(rv, bn64.running_var, bn32.running_var, 'running_var')


# ---------------------------------------------------------------------------------------------------------------------------------
# whole network
# ---------------------------------------------------------------------------------------------------------------------------------
SMALL = OrderedDict(layer5=32, layer4=16, layer3=8, layer2=8)
RN101 = OrderedDict(layer5=2048, layer4=1024, layer3=512, layer2=256)


def _net(chans, use_bn, seed=1, oc=64):
    from frtm_vos_amd.model.seg_network import SegNetwork
    torch.manual_seed(seed)
    net = SegNetwork(1, oc, chans, use_bn)
    g = torch.Generator().manual_seed(seed + 7)
    with torch.no_grad():
        for name, b in net.named_buffers():
            if name.endswith('running_var'):
                b.copy_(torch.rand(b.shape, generator=g) + 0.5)
            elif name.endswith('running_mean'):
                b.copy_(torch.randn(b.shape, generator=g) * 0.1)
        for name, p in net.named_parameters():
            if name.endswith('bias'):
                p.add_(torch.randn(p.shape, generator=g) * 0.05)
    return net


def _inputs(chans, B, Hh, Ww, seed=2):
    g = torch.Generator().manual_seed(seed)
    feats = {}
    for i, (L, c) in enumerate(chans.items()):
        s = 32 >> i
        feats[L] = torch.relu(torch.randn(B, c, (Hh + s - 1) // s, (Ww + s - 1) // s, generator=g))
    scores = torch.randn(B, 1, feats['layer4'].shape[2], feats['layer4'].shape[3], generator=g)
    return scores, feats


def _run(net, scores, feats, size, hip, dl):
    for p in net.parameters():
        p.grad = None
    out = net.forward_train(scores, feats, size) if hip else net.forward_torch(scores, feats, size)
    out.backward(dl)
    return out.detach(), {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None}


def _compare_network(chans, use_bn, B, Hh, Ww, train, steps=1):
    net = _net(chans, use_bn).train(train)
    scores, feats = _inputs(chans, B, Hh, Ww)
    g = torch.Generator().manual_seed(9)
    m64 = copy.deepcopy(net).double()
    m32 = copy.deepcopy(net).to(DEV)
    mh = copy.deepcopy(net).to(DEV)
    ratios = []
    for step in range(steps):
        dl = torch.randn(B, 1, Hh, Ww, generator=g, dtype=torch.float64)
        o64, g64 = _run(m64, scores.double(), {k: v.double() for k, v in feats.items()}, (Hh, Ww), False, dl)
        fd = {k: v.to(DEV) for k, v in feats.items()}
        o32, g32 = _run(m32, scores.to(DEV), fd, (Hh, Ww), False, dl.float().to(DEV))
        oh, gh = _run(mh, scores.to(DEV), fd, (Hh, Ww), True, dl.float().to(DEV))
        ratios.append(_gate(oh, o64, o32, 'logits'))
        assert set(gh) == set(g64)
        for k in g64:
            floor = None
            if use_bn and k.endswith('bblock.0.bias') and train:       # analytically zero under batch statistics
                floor = 1e-5 * float(g64[k.replace('bias', 'weight')].abs().max())
            ratios.append(_gate(gh[k], g64[k], g32[k], k, floor=floor))
    for (k, b64), b32, bh in zip(m64.named_buffers(), m32.buffers(), mh.buffers()):
        if k.endswith('num_batches_tracked'):
            assert int(bh) == int(b64) == (steps if (use_bn and train) else 0), k
        elif k.startswith(('TSE', 'RRB', 'CAB')):
            _gate(bh, b64, b32, k)
    return max(ratios)


@pytest.mark.parametrize('use_bn', [True, False])
@pytest.mark.parametrize('train', [True, False])
def test_network_small(use_bn, train):
    r = _compare_network(SMALL, use_bn, 2, 96, 160, train, steps=3 if train else 1)
    print('max gate ratio %.3f' % r)


def test_network_rn101_480p():
    r = _compare_network(RN101, True, 2, 480, 854, True)
    print('max gate ratio %.3f' % r)


def test_eval_logits_match_inference_forward():
    net = _net(SMALL, True).to(DEV).eval()
    scores, feats = _inputs(SMALL, 2, 96, 160)
    scores, feats = scores.to(DEV), {k: v.to(DEV) for k, v in feats.items()}
    a = net.forward_train(scores, feats, (96, 160)).detach()
    with torch.no_grad():
        b = net(scores, feats, (96, 160))
    assert float((a - b).abs().max()) < 1e-3 * float(b.abs().max()) + 1e-4


def test_determinism_b16_480p():
    net = _net(RN101, True).to(DEV).train()
    scores, feats = _inputs(RN101, 16, 480, 854)
    scores, feats = scores.to(DEV), {k: v.to(DEV) for k, v in feats.items()}
    dl = torch.randn(16, 1, 480, 854, generator=torch.Generator().manual_seed(4)).to(DEV) * 1e-3
    bufs = {k: b.clone() for k, b in net.named_buffers()}
    _, g1 = _run(net, scores, feats, (480, 854), True, dl)
    b1 = {k: b.clone() for k, b in net.named_buffers()}
    with torch.no_grad():
        for k, b in net.named_buffers():
            b.copy_(bufs[k])
    _, g2 = _run(net, scores, feats, (480, 854), True, dl)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    for k, b in net.named_buffers():
        assert torch.equal(b, b1[k]), k
    with torch.no_grad():
        for k, b in net.named_buffers():
            b.copy_(bufs[k])
    # values: the same fp64 gate as the small cases, with the float64 reference computed on the GPU (an fp64 CPU pass at this size takes
    # minutes).  A comparison with the fp32 PyTorch path alone cannot gate at this size: that path is itself up to 2.4e-2 of max|g| away
    # from fp64 here (HIP: 7.5e-3), the gradients behind the ReLU masks and batch statistics of 16 frames being that sensitive.
    m64 = copy.deepcopy(net).double()
    m32 = copy.deepcopy(net)
    _, g64 = _run(m64, scores.double(), {k: v.double() for k, v in feats.items()}, (480, 854), False, dl.double())
    _, g32 = _run(m32, scores, feats, (480, 854), False, dl)
    ratios = []
    for k in g64:
        floor = 1e-5 * float(g64[k.replace('bias', 'weight')].abs().max()) if k.endswith('bblock.0.bias') else None   # analytically zero
        ratios.append(_gate(g1[k], g64[k], g32[k], k, floor=floor))
    print('max gate ratio %.3f' % max(ratios))


def test_no_framework_compute(monkeypatch):
    net = _net(SMALL, True).to(DEV).train()
    scores, feats = _inputs(SMALL, 2, 96, 160)
    scores, feats = scores.to(DEV), {k: v.to(DEV) for k, v in feats.items()}

    def boom(*a, **k):
        raise AssertionError('framework compute in forward_train')
    for name in ('conv2d', 'batch_norm', 'interpolate', 'leaky_relu'):
        monkeypatch.setattr(F, name, boom)
    monkeypatch.setattr(torch, 'conv2d', boom)
    out = net.forward_train(scores, feats, (96, 160))
    out.sum().backward()
    assert all(p.grad is not None for p in net.parameters())


def test_frozen_submodule():
    net = _net(SMALL, True).to(DEV).train()
    scores, feats = _inputs(SMALL, 2, 96, 160)
    scores, feats = scores.to(DEV), {k: v.to(DEV) for k, v in feats.items()}
    dl = torch.randn(2, 1, 96, 160, device=DEV)
    bufs = {k: b.clone() for k, b in net.named_buffers()}
    _, full = _run(net, scores, feats, (96, 160), True, dl)
    with torch.no_grad():
        for k, b in net.named_buffers():
            b.copy_(bufs[k])
    net.TSE['layer3'].requires_grad_(False)
    net.project.conv2.requires_grad_(False)
    _, part = _run(net, scores, feats, (96, 160), True, dl)
    for k, p in net.named_parameters():
        if k.startswith('TSE.layer3.') or k.startswith('project.conv2.'):
            assert p.grad is None, k
        else:
            assert torch.equal(part[k], full[k]), k


def test_refusals_on_gpu():
    from frtm_vos_amd.model.seg_network import SegNetwork
    net = _net(SMALL, True).to(DEV)
    scores, feats = _inputs(SMALL, 2, 96, 160)
    scores, feats = scores.to(DEV), {k: v.to(DEV) for k, v in feats.items()}
    with pytest.raises(ValueError):
        net.forward_train(torch.cat([scores, scores]), feats, (96, 160))
    with pytest.raises(ValueError):
        net.forward_train(scores.clone().requires_grad_(), feats, (96, 160))
    with pytest.raises(NotImplementedError, match='forward_torch'):
        SegNetwork(1, 8, SMALL, True, upsampler='bicubic').to(DEV).forward_train(scores, feats, (96, 160))


def test_trainer_model_hip_backend(tmp_path):
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    from frtm_vos_amd.model.augmenter import ImageAugmenter
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    from frtm_vos_amd.model.seg_network import SegNetwork
    from frtm_vos_amd.model.training_model import SampleSpec, TrainerModel
    P = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18')
    P.disc_params.update(memory_size=20, init_iters=(3, 5), update_iters=(3,), c_channels=32)
    ext = ResnetFeatureExtractor('resnet18').to(DEV)
    chans = {L: n for L, n in ext.get_out_channels().items() if L in P.refnet_params.layers}
    torch.manual_seed(1)
    init = SegNetwork(1, 64, chans, True).to(DEV)
    seqs = [SyntheticSequence('s%d' % k, 3, (128, 160), 1, seed=30 + k) for k in range(2)]
    images = [torch.stack([s.images[t] for s in seqs]) for t in range(3)]
    labels = [torch.stack([(s.gt[t] == 1).to(torch.uint8) for s in seqs]) for t in range(3)]
    meta = [SampleSpec('s%d' % k, 1, ['00000', '00001', '00002'], 0).encoded() for k in range(2)]
    runs = {}
    for backend in ('torch', 'hip'):
        refiner = copy.deepcopy(init)
        m = TrainerModel(ImageAugmenter(P.aug_params), ext, P.disc_params, refiner, batch_size=2,
                         tmodel_cache=dict(path=tmp_path / 'cache', enable=True, read_only=False), device=DEV, refiner_backend=backend)
        __import__('numpy').random.seed(0)
        opt = torch.optim.Adam(refiner.parameters(), lr=1e-3)
        losses, grads, hits = [], None, []
        for step in range(5):
            opt.zero_grad()
            st = m(images, labels, meta)
            losses.append(st['stats/loss'])
            hits.append(st['stats/fcache_hits'])
            if step == 0:
                grads = {k: p.grad.clone() for k, p in refiner.named_parameters()}
            opt.step()
        runs[backend] = (losses, grads, hits)
    lt, gt, ht = runs['torch']
    lh, gh, hh = runs['hip']
    assert ht == [0, 2, 2, 2, 2] and hh == [2] * 5            # the second backend reads the first one's cache
    assert abs(lh[0] - lt[0]) <= 1e-4 * lt[0]
    for k in gt:
        floor = 1e-3 * float(gt[k.replace('bias', 'weight')].abs().max()) if k.endswith('bblock.0.bias') else 0.0   # analytically zero
        assert _err(gh[k], gt[k]) <= max(1e-3 * float(gt[k].abs().max()), floor), k
    assert lh[-1] < lh[0] and lt[-1] < lt[0]
    assert abs(lh[-1] - lt[-1]) <= 0.01 * lt[-1]
    with pytest.raises(ValueError):
        TrainerModel(ImageAugmenter(P.aug_params), ext, P.disc_params, init, batch_size=2, refiner_backend='bogus')
