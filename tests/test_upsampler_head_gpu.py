"""GPU tests of the bicubic refiner head (model/seg_network.py: Upsampler): the two HIP kernels (frtm_bicubic_resize,
frtm_project_tail_bicubic) against PyTorch and against each other, SegNetwork(upsampler='bicubic') on the HIP path against its PyTorch
definition and fixture G19, in one stream, with side-stream levels and replayed as a graph, and a tracker built with the head."""
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
T = torch.from_numpy
DEV = 'cuda:0'


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _resize(x, H, W):
    from frtm_vos_amd import _hip as Hh
    p, h, w = x.shape
    out = torch.empty(p, H, W, device=DEV)
    Hh.call('frtm_bicubic_resize', Hh.ptr(x), p, h, w, Hh.ptr(out), H, W)
    return out


def _tail(y, w3, b, Ho, Wo):
    from frtm_vos_amd import _hip as Hh
    n, C, h, w = y.shape
    out = torch.empty(n, 1, Ho, Wo, device=DEV)
    Hh.call('frtm_project_tail_bicubic', Hh.ptr(y), n, C, h, w, Hh.ptr(w3), Hh.ptr(b), Ho, Wo, Hh.ptr(out))
    return out


def _unfused(y, w3, b, Ho, Wo):
    from frtm_vos_amd import ops
    n, C, h, w = y.shape
    z = _resize(y.reshape(n * C, h, w), Ho, Wo).reshape(n, C, Ho, Wo)
    return ops.filter_scores(z, w3, out=b.view(1, 1, 1, 1).expand(n, 1, Ho, Wo).contiguous(), accumulate=True)


@pytest.mark.parametrize('h,w,H,W', [(15, 27, 30, 54), (60, 107, 120, 214), (120, 214, 480, 854), (120, 214, 720, 1280),
                                     (270, 480, 1080, 1920), (480, 854, 120, 214), (1, 5, 3, 17)])
def test_bicubic_resize_vs_interpolate(h, w, H, W):
    x = torch.randn(3, h, w, generator=gen(h * 7 + w))
    ref = F.interpolate(x[None], (H, W), mode='bicubic', align_corners=False)[0]
    out = _resize(x.to(DEV), H, W)
    assert out.shape == ref.shape
    assert rel(out, ref) <= 1e-5, rel(out, ref)


@pytest.mark.parametrize('h,w', [(15, 27), (120, 214), (7, 3)])
def test_pyrup2x_is_the_2x_bicubic_resize(h, w):
    """The head's first step runs on frtm_pyrup2x (model/seg_network.py: SegNetwork._forward_hip): at exactly 2x it is the same operator
    as the bicubic resize, to rounding."""
    from frtm_vos_amd import _hip as Hh
    x = torch.randn(4, h, w, generator=gen(5)).to(DEV)
    up = torch.empty(4, 2 * h, 2 * w, device=DEV)
    Hh.call('frtm_pyrup2x', Hh.ptr(x), 4, h, w, Hh.ptr(up))
    assert rel(up, _resize(x, 2 * h, 2 * w)) <= 1e-6


@pytest.mark.parametrize('H,W', [(480, 854), (720, 1280), (1080, 1920), (473, 851)])
def test_project_tail_bicubic_fused_vs_unfused(H, W):
    """frtm_project_tail_bicubic == frtm_bicubic_resize + frtm_filter_scores on the 2x layer2 map of an H x W frame, on conv1's 32
    channels and on the nine tap maps of frtm_tap_mix with one-hot weights (the form SegNetwork runs)."""
    from frtm_vos_amd import _hip as Hh
    from frtm_vos_amd.model.seg_network import bicubic_tail_fits
    h, w = 2 * ((H + 3) // 4), 2 * ((W + 3) // 4)
    assert bicubic_tail_fits(h, w, H, W)
    g = gen(H + W)
    n = 2
    y = torch.relu(torch.randn(n, 32, h, w, generator=g)).to(DEV)
    w3 = (torch.randn(1, 32, 3, 3, generator=g) * 0.2).to(DEV)
    b = torch.tensor([0.3], device=DEV)
    fused = _tail(y, w3, b, H, W)
    assert rel(fused, _unfused(y, w3, b, H, W)) <= 1e-5, rel(fused, _unfused(y, w3, b, H, W))
    ym = torch.empty(n, 9, h, w, device=DEV)
    Hh.call('frtm_tap_mix', Hh.ptr(y), n, 32, h * w, Hh.ptr(w3), Hh.ptr(ym))
    eye9 = torch.eye(9, device=DEV).contiguous()
    mixed = _tail(ym, eye9, b, H, W)
    assert rel(mixed, _unfused(ym, eye9, b, H, W)) <= 1e-5
    assert rel(mixed, fused) <= 1e-5
    if H == 480:         # and the definition itself (PyTorch on the CPU)
        ref = F.conv2d(F.interpolate(y.cpu(), (H, W), mode='bicubic', align_corners=False), w3.cpu(), b.cpu(), padding=1)
        assert rel(fused, ref) <= 1e-5, rel(fused, ref)


def test_project_tail_bicubic_ratio_check_and_fallback():
    """Outside its LDS patch the fused kernel refuses (FRTM_ERR_ARG); bicubic_tail_fits predicts the refusal, and SegNetwork then composes
    frtm_bicubic_resize + frtm_filter_scores: the same result as with fuse_tail off."""
    from frtm_vos_amd.model.seg_network import SegNetwork, bicubic_tail_fits
    y = torch.zeros(1, 2, 64, 64, device=DEV)
    w3 = torch.zeros(1, 2, 3, 3, device=DEV)
    with pytest.raises(RuntimeError, match='resize ratio'):
        _tail(y, w3, None, 80, 80)
    for (h, w, Ho, Wo) in [(64, 64, 80, 80), (28, 38, 48, 70), (28, 38, 48, 74), (240, 428, 480, 854), (30, 30, 50, 300), (30, 30, 300, 50),
                           (20, 37, 41, 70), (20, 37, 41, 71), (8, 8, 128, 128)]:
        yy = torch.zeros(1, 1, h, w, device=DEV)
        ww = torch.zeros(1, 1, 3, 3, device=DEV)
        if bicubic_tail_fits(h, w, Ho, Wo):
            _tail(yy, ww, None, Ho, Wo)
        else:
            with pytest.raises(RuntimeError, match='resize ratio'):
                _tail(yy, ww, None, Ho, Wo)
    chans = OrderedDict(layer5=40, layer4=24, layer3=16, layer2=8)
    torch.manual_seed(7)
    net = SegNetwork(1, 8, chans, True, upsampler='bicubic').eval().to(DEV)
    g = gen(29)
    size, dims = (48, 70), [(2, 3), (4, 5), (7, 10), (14, 19)]         # 2x layer2 = 28 x 38: outside the patch
    assert not bicubic_tail_fits(28, 38, *size)
    feats = {L: torch.relu(torch.randn(1, c, *d, generator=g)).to(DEV) for (L, c), d in zip(chans.items(), dims)}
    scores = torch.randn(2, 1, *dims[1], generator=g).to(DEV)
    with torch.no_grad():
        out = net(scores, feats, size)
        net.fuse_tail = False
        unfused = net(scores, feats, size)
        ref = net.forward_torch(scores, feats, size)
    assert torch.equal(out, unfused)
    assert rel(out, ref) < 2e-4, rel(out, ref)


def _perturb_bn(net):
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.5, 1.5); m.weight.data.uniform_(0.5, 1.5); m.bias.data.normal_(0, 0.2)


def test_segnetwork_bicubic_hip_vs_torch():
    """RN101 widths, 480 x 854, two objects: the HIP head (fused tail on the tap maps, and the unfused forms) == forward_torch."""
    from frtm_vos_amd.model.seg_network import SegNetwork
    chans = OrderedDict(layer5=2048, layer4=1024, layer3=512, layer2=256)
    torch.manual_seed(3)
    net = SegNetwork(1, 64, chans, True, upsampler='bicubic').eval()
    _perturb_bn(net)
    g = gen(17)
    size, n = (480, 854), 2
    dims = [((size[0] + 2 ** k - 1) // 2 ** k, (size[1] + 2 ** k - 1) // 2 ** k) for k in (5, 4, 3, 2)]
    feats = {L: torch.relu(torch.randn(1, c, *d, generator=g)).to(DEV) for (L, c), d in zip(chans.items(), dims)}
    scores = torch.randn(n, 1, *dims[1], generator=g).to(DEV)
    net = net.to(DEV)
    with torch.no_grad():
        ref = net.forward_torch(scores, feats, size)
        for fuse, mix in ((True, True), (True, False), (False, True)):
            net.fuse_tail, net.mix_taps = fuse, mix
            hip = net(scores, feats, size)
            assert hip.shape == (n, 1) + size
            assert rel(hip, ref) < 2e-4, (fuse, mix, rel(hip, ref))


def test_segnetwork_bicubic_frame_window():
    """A window of 3 frames x 2 objects == per-frame calls: eagerly on one stream, with the deep levels on the side stream, and replayed
    as a graph."""
    from frtm_vos_amd.model.seg_network import SegNetwork
    chans = OrderedDict(layer5=40, layer4=24, layer3=16, layer2=8)
    torch.manual_seed(5)
    net = SegNetwork(1, 8, chans, True, upsampler='bicubic').eval().to(DEV)
    g = gen(19)
    size, Fn, n = (93, 137), 3, 2
    dims = [((size[0] + 2 ** k - 1) // 2 ** k, (size[1] + 2 ** k - 1) // 2 ** k) for k in (5, 4, 3, 2)]
    feats = {L: torch.relu(torch.randn(Fn, c, *d, generator=g)).to(DEV) for (L, c), d in zip(chans.items(), dims)}
    scores = torch.randn(Fn * n, 1, *dims[1], generator=g).to(DEV)
    with torch.no_grad():
        ref = net.forward_torch(scores, feats, size)
        one = torch.cat([net(scores[f * n:(f + 1) * n], {L: t[f:f + 1] for L, t in feats.items()}, size) for f in range(Fn)])
        assert rel(one, ref) < 2e-4
        for parallel in (False, True):
            net.parallel_eager = parallel
            win = net(scores, feats, size)
            assert rel(win, one) < 1e-5, parallel
        net.use_graphs = True
        for _ in range(3):                      # launched, captured + replayed, replayed
            assert rel(net(scores, feats, size), one) < 1e-5


def test_swapping_the_head_reaches_the_hip_path():
    """net.project = Upsampler(...) after construction (the reference's commented-out line): the next HIP call, eager or replayed, runs
    the new head."""
    from frtm_vos_amd.lib.synthetic import make_score_following_refiner
    from frtm_vos_amd.model.seg_network import SegNetwork, Upsampler
    chans = OrderedDict(layer5=40, layer4=24, layer3=16, layer2=8)
    torch.manual_seed(9)
    net = make_score_following_refiner(SegNetwork(1, 8, chans, True).eval()).to(DEV)
    g = gen(21)
    size = (93, 137)                      # not 4x the layer2 map: the two heads differ (at exactly 4x they coincide)
    dims = [((size[0] + 2 ** k - 1) // 2 ** k, (size[1] + 2 ** k - 1) // 2 ** k) for k in (5, 4, 3, 2)]
    feats = {L: torch.relu(torch.randn(1, c, *d, generator=g)).to(DEV) for (L, c), d in zip(chans.items(), dims)}
    scores = torch.randn(2, 1, *dims[1], generator=g).to(DEV)
    net.use_graphs = True
    with torch.no_grad():
        for _ in range(3):
            compat = net(scores, feats, size).clone()
        head = Upsampler(8).to(DEV)
        head.load_state_dict(net.project.state_dict())
        net.project = head
        ref = net.forward_torch(scores, feats, size)
        for _ in range(3):
            out = net(scores, feats, size)
            assert rel(out, ref) < 2e-4
    assert float((out - compat).abs().max()) > 1e-3, float((out - compat).abs().max())


def test_hip_refiner_on_g19(golden):
    """The HIP refiner with the bicubic head on fixture G19's inputs (case A: fused tail; case B: outside the patch, the fallback)."""
    from frtm_vos_amd.model.seg_network import SegNetwork, bicubic_tail_fits
    from test_upsampler_head import CHANS, _keyed_state_dict          # (tests/ is on the path: pytest's rootdir-less import mode)
    g = golden('g19_upsampler')
    net = SegNetwork(1, 8, CHANS, True, upsampler='bicubic').eval()
    net.load_state_dict(_keyed_state_dict(net))
    net = net.to(DEV)
    fits = []
    for tag in ('A', 'B'):
        feats = {L: T(g['%s_ft_%s' % (tag, L)]).to(DEV) for L in CHANS}
        size = tuple(int(v) for v in g[tag + '_size'])
        h2, w2 = 2 * feats['layer2'].shape[-2], 2 * feats['layer2'].shape[-1]
        fits.append(bicubic_tail_fits(h2, w2, *size))
        with torch.no_grad():
            out = net(T(g[tag + '_scores']).to(DEV), feats, size)
        assert rel(out, T(g[tag + '_out'])) < 2e-4, (tag, rel(out, T(g[tag + '_out'])))
    assert fits == [True, False]


def test_tracker_with_bicubic_head():
    """Parameters(upsampler='bicubic') end to end: run_sequence (batched trunk, windows) == the literal per-frame track() loop, and the
    head really is the bicubic one (its refiner output differs from the compat head's on the same weights).  The refiners are turned into
    the score-following stand-in for a trained one (confident masks, so that the memory updates and re-solves run), and the frame size is
    not 4x the layer2 map (at exactly 4x the two heads coincide: the compat head's bilinear step is then the identity)."""
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence, make_score_following_refiner
    from frtm_vos_amd.model.seg_network import SegNetwork, Upsampler
    from frtm_vos_amd import ops as O_

    def make():
        torch.manual_seed(0)
        params = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18', feature_batch=8, upsampler='bicubic')
        params.disc_params.update(memory_size=8, init_iters=(2, 3), update_iters=(3,))
        trk = params.get_model().eval()
        make_score_following_refiner(trk.refiner)
        return trk

    size = (122, 170)
    seq = SyntheticSequence('bic', 13, size, 2, seed=5)
    seq.preload(DEV)
    trk_fast = make()
    assert isinstance(trk_fast.refiner.project, Upsampler)
    soft_fast = []
    tw = trk_fast.track_window
    trk_fast.track_window = lambda images, taps: (lambda m: (soft_fast.extend(m.clone().unbind(0)), m)[1])(tw(images, taps))
    fast, _ = trk_fast.run_sequence(seq)
    fast = torch.stack([l.reshape(*size) for l in fast]).cpu()
    trk = make()
    ids = torch.tensor([0] + list(seq.obj_ids), dtype=torch.uint8, device=DEV)
    slow, soft_slow = [], []
    for i, (image, labels, new_objects) in enumerate(seq):
        image = image.to(DEV)
        had = len(trk.targets) > 0
        if len(new_objects) > 0:
            trk.initialize(image, labels.to(DEV), new_objects)
        if had:
            masks = trk.track(image)
            soft_slow.append(masks.clone())
            labels = ids[O_.merge_masks_(masks.clone()).argmax(dim=0, keepdim=True)]
        slow.append(labels.reshape(*size).cpu())
        trk.current_frame += 1
    slow = torch.stack(slow)
    agree = float((fast == slow).float().mean())
    assert agree > 0.995, agree
    assert len(soft_fast) == len(soft_slow) == 12
    d = max(float((a - b).abs().mean()) for a, b in zip(soft_fast, soft_slow))
    assert d < 2e-3, d
    # the same weights through the compat head: a different model
    ref = trk.refiner
    compat = SegNetwork(1, 64, ref.ft_channels, True).eval().to(DEV)
    compat.load_state_dict(ref.state_dict())
    g = gen(3)
    dims = [((size[0] + 2 ** k - 1) // 2 ** k, (size[1] + 2 ** k - 1) // 2 ** k) for k in (5, 4, 3, 2)]
    feats = {L: torch.relu(torch.randn(2, c, *d, generator=g)).to(DEV) for (L, c), d in zip(ref.ft_channels.items(), dims)}
    scores = torch.randn(4, 1, *dims[1], generator=g).to(DEV)
    with torch.no_grad():
        a, b = ref(scores, feats, size), compat(scores, feats, size)
    assert float((a - b).abs().max()) > 1e-3, float((a - b).abs().max())
