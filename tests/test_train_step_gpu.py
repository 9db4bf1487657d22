"""The ends of the training step on the GPU (csrc/train_step.hip): the loss tail against both fp64 definitions, FusedAdam against
torch.optim.Adam, the absence of framework compute and of per-frame read-backs in TrainerModel(loss_backend='hip'), the whole step
against the parent path, and the driver (lib/training.py, train.py) resuming bit for bit.

Gate (per tensor, the one of tests/test_refiner_train_gpu.py): max|hip - ref64| <= max(4 * max|torch32 - ref64|, 1e-6 * max|ref64|),
ref64 = PyTorch in float64, torch32 = the same ops in fp32 on the GPU."""
import copy
import os
import subprocess
import sys
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _grad_mode_on():
    prev = torch.is_grad_enabled()
    torch.set_grad_enabled(True)
    yield
    torch.set_grad_enabled(prev)


def _err(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def _gate(hip, ref64, t32, what):
    e, e32 = _err(hip, ref64), _err(t32, ref64)
    bound = max(4 * e32, 1e-6 * float(ref64.detach().abs().max()))
    print('%s: hip err %.3e, torch32 err %.3e, bound %.3e, err/bound %.3f' % (what, e, e32, bound, e / max(bound, 1e-300)))
    assert e <= bound, '%s: hip err %.3e, torch32 err %.3e, bound %.3e' % (what, e, e32, bound)
    return e / max(bound, 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the loss kernel
# ---------------------------------------------------------------------------------------------------------------------------------
def _bce_sigmoid(z, t):
    return F.binary_cross_entropy(torch.sigmoid(z), t)


def _logits(shape, std, clamp, seed):
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(shape, generator=g) * std).clamp(-clamp, clamp)
    # 6.5 million normal draws do come closer to 0 than 1e-6 (about five of them at std 1): those few are moved out to +-1e-3
    z = torch.where(z.abs() < 1e-3, torch.where(z < 0, -1e-3, 1e-3).to(z.dtype), z)
    assert float(z.abs().min()) >= 1e-6                      # no logit sits on the threshold: the counts below are exact in any precision
    return z


def _targets(shape, kind, seed):
    g = torch.Generator().manual_seed(seed + 100)
    if kind == 'soft':
        t = torch.rand(shape, generator=g)
        assert float((t - 0.5).abs().min()) > 0
        return t
    t = torch.rand(shape, generator=g) < 0.3
    return t.to(torch.uint8) if kind == 'u8' else t.float()


def _reference(fn, z, t):
    z64 = z.double().requires_grad_()
    l64 = fn(z64, t.double())
    l64.backward()
    z32 = z.to(DEV).requires_grad_()
    l32 = fn(z32, t.float().to(DEV))
    l32.backward()
    return l64.detach(), z64.grad, l32.detach(), z32.grad


SIZES = [(2, 1, 96, 160), (3, 1, 37, 45), (16, 1, 480, 854)]
DEFS = [('sigmoid', 1.0), ('sigmoid', 4.0), ('sigmoid', 8.0), ('with_logits', 30.0)]


@pytest.mark.parametrize('shape', SIZES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('definition,std', DEFS)
@pytest.mark.parametrize('kind', ['u8', 'f32'])
def test_loss_kernel_against_fp64(shape, definition, std, kind):
    from frtm_vos_amd import ops
    fn, clamp = (_bce_sigmoid, 15.0) if definition == 'sigmoid' else (F.binary_cross_entropy_with_logits, 90.0)
    z, t = _logits(shape, std, clamp, seed=int(std) + shape[2]), _targets(shape, kind, seed=shape[3])
    l64, d64, l32, d32 = _reference(fn, z, t)
    loss, dz, inter, union = ops.bce_logits(z.to(DEV), t.to(DEV))
    assert loss.dtype == torch.float32 and loss.dim() == 0 and inter.dtype == union.dtype == torch.int32
    _gate(loss, l64, l32, 'loss')
    _gate(dz, d64, d32, 'dz')
    p, g = z.double() > 0, t.double() > 0.5
    assert torch.equal(inter.cpu().long(), (p & g).flatten(1).sum(1)) and torch.equal(union.cpu().long(), (p | g).flatten(1).sum(1))
    again = ops.bce_logits(z.to(DEV), t.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip((loss, dz, inter, union), again))            # bit for bit
    only = ops.bce_logits(z.to(DEV), t.to(DEV), grad=False)                                        # evaluation: no gradient written
    assert only[1] is None and torch.equal(only[0], loss) and torch.equal(only[2], inter) and torch.equal(only[3], union)


@pytest.mark.parametrize('shape', SIZES[:2], ids=lambda s: 'x'.join(map(str, s)))
def test_loss_kernel_soft_targets(shape):
    from frtm_vos_amd import ops
    z, t = _logits(shape, 4.0, 15.0, seed=5), _targets(shape, 'soft', seed=6)
    l64, d64, l32, d32 = _reference(_bce_sigmoid, z, t)
    loss, dz, inter, union = ops.bce_logits(z.to(DEV), t.to(DEV))
    _gate(loss, l64, l32, 'loss')
    _gate(dz, d64, d32, 'dz')
    p, g = z.double() > 0, t.double() > 0.5
    assert torch.equal(inter.cpu().long(), (p & g).flatten(1).sum(1)) and torch.equal(union.cpu().long(), (p | g).flatten(1).sum(1))


def test_loss_kernel_clamp_at_100():
    """Three hand-placed pixels beyond |z| = 100: a wrong one contributes exactly 100 and no gradient (BCELoss's log clamp), a right
    one nothing."""
    from frtm_vos_amd import ops
    z = torch.full((1, 1, 3, 5), -2.0)
    t = torch.zeros(1, 1, 3, 5)
    z[0, 0, 0, 1], t[0, 0, 0, 1] = 150.0, 0.0            # confidently wrong: clamp binds
    z[0, 0, 1, 2], t[0, 0, 1, 2] = -150.0, 1.0           # confidently wrong the other way
    z[0, 0, 2, 4], t[0, 0, 2, 4] = 150.0, 1.0            # confidently right
    loss, dz, inter, union = ops.bce_logits(z.to(DEV), t.to(DEV))
    rest = float(F.softplus(torch.tensor(-2.0, dtype=torch.float64))) * 12
    assert abs(float(loss) - (200.0 + rest) / 15) <= 1e-6 * (200.0 + rest) / 15
    dz = dz.cpu()
    assert float(dz[0, 0, 0, 1]) == 0.0 and float(dz[0, 0, 1, 2]) == 0.0 and float(dz[0, 0, 2, 4]) == 0.0
    assert abs(float(dz[0, 0, 0, 0]) - float(torch.sigmoid(torch.tensor(-2.0, dtype=torch.float64))) / 15) < 1e-8
    assert inter.tolist() == [1] and union.tolist() == [3]


def test_loss_function_autograd_and_refusals():
    from frtm_vos_amd.model.train_loss import bce_logits_stats, iou_from_counts
    from frtm_vos_amd.model.training_model import mask_iou
    z, t = _logits((3, 1, 37, 45), 4.0, 15.0, seed=8), _targets((3, 1, 37, 45), 'u8', seed=9)
    w = torch.full((), 0.7, device=DEV, requires_grad=True)
    x = z.to(DEV)
    loss, inter, union = bce_logits_stats(x * w, t.to(DEV))               # logits with a torch grad_fn behind them
    assert not inter.requires_grad and not union.requires_grad
    (loss * 0.5).backward()                                               # the incoming scalar is applied on the device
    z64 = z.double()
    w64 = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    (_bce_sigmoid(z64 * w64, t.double()) * 0.5).backward()
    assert abs(float(w.grad) - float(w64.grad)) <= 1e-5 * abs(float(w64.grad))
    assert torch.allclose(iou_from_counts(inter, union), mask_iou(torch.sigmoid(x * 0.7), t.to(DEV).float()).flatten())
    empty = iou_from_counts(torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    assert empty.tolist() == [1.0, 1.0]                                   # mask_iou's convention
    with pytest.raises(ValueError, match='differ in size'):
        bce_logits_stats(x, t.to(DEV)[:, :, :30])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bce_logits_stats(x, t)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. FusedAdam
# ---------------------------------------------------------------------------------------------------------------------------------
SMALL = OrderedDict(layer5=32, layer4=16, layer3=8, layer2=8)
RN101 = OrderedDict(layer5=2048, layer4=1024, layer3=512, layer2=256)
NO_GRAD = 5                     # index of the parameter that never receives a gradient


def _refiner_params(chans):
    from frtm_vos_amd.model.seg_network import SegNetwork
    torch.manual_seed(1)
    return [p.detach().clone() for p in SegNetwork(1, 64, chans, True).parameters()]


def _grads(init, steps, seed=11):
    """steps x tensors seeded fp32 gradients, their scale spread per tensor over 1e-4 ... 1."""
    g = torch.Generator().manual_seed(seed)
    scales = [10.0 ** (-4.0 * ((7 * k) % len(init)) / max(len(init) - 1, 1)) for k in range(len(init))]
    return [[torch.randn(p.shape, generator=g) * s for p, s in zip(init, scales)] for _ in range(steps)]


def _optimise(kind, init, grads, amsgrad, state=None):
    """kind: 'ref64' (torch Adam, fp64, CPU), 'torch32' (torch Adam, fp32, GPU), 'hip' (FusedAdam); state: (optimiser, scheduler) state
    dicts to continue from.  Returns (params, optimiser, scheduler)."""
    from frtm_vos_amd.lib.fused_adam import FusedAdam
    dev, dt = ('cpu', torch.float64) if kind == 'ref64' else (DEV, torch.float32)
    params = [torch.nn.Parameter(p.to(dev, dt)) for p in init]
    cls = FusedAdam if kind == 'hip' else torch.optim.Adam
    opt = cls(params, lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-5, amsgrad=amsgrad)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=7, gamma=0.1)
    if state is not None:
        opt.load_state_dict(copy.deepcopy(state[0]))
        sched.load_state_dict(copy.deepcopy(state[1]))
    for gs in grads:
        for k, (p, g) in enumerate(zip(params, gs)):
            p.grad = None if k == NO_GRAD else g.to(dev, dt)
        opt.step()
        sched.step()
    return params, opt, sched


def _gate_optimiser(hip, ref, t32, what):
    (ph, oh), (p64, o64), (p32, o32) = hip[:2], ref[:2], t32[:2]
    worst = 0.0
    for k in range(len(p64)):
        worst = max(worst, _gate(ph[k], p64[k], p32[k], '%s param %d' % (what, k)))
        assert set(oh.state.get(ph[k], {})) == set(o64.state.get(p64[k], {}))
        for name in o64.state.get(p64[k], {}):
            if name == 'step':
                assert float(oh.state[ph[k]]['step']) == float(o64.state[p64[k]]['step'])
            else:
                worst = max(worst, _gate(oh.state[ph[k]][name], o64.state[p64[k]][name], o32.state[p32[k]][name], '%s %s %d' % (what, name, k)))
    return worst


@pytest.mark.parametrize('chans', [SMALL, RN101], ids=['small', 'rn101'])
@pytest.mark.parametrize('amsgrad', [True, False])
def test_fused_adam_against_torch(chans, amsgrad):
    init = _refiner_params(chans)
    if chans is RN101:
        assert len(init) == 116 and sum(p.numel() for p in init) == 1410449
        assert sum(p.numel() % 4 != 0 for p in init) == 17 and min(p.numel() for p in init) == 1
    grads = _grads(init, 20)
    runs = {kind: _optimise(kind, init, grads, amsgrad) for kind in ('hip', 'ref64', 'torch32')}
    print('worst err/bound %.3f' % _gate_optimiser(runs['hip'], runs['ref64'], runs['torch32'], 'adam'))
    ph, oh, _ = runs['hip']
    assert torch.equal(ph[NO_GRAD].detach().cpu(), init[NO_GRAD]) and len(oh.state.get(ph[NO_GRAD], {})) == 0     # skipped as torch skips it
    assert oh.param_groups[0]['lr'] == pytest.approx(1e-5)                                               # StepLR(7) stepped twice in 20
    ph2, oh2, _ = _optimise('hip', init, grads, amsgrad)
    for a, b in zip(ph, ph2):
        assert torch.equal(a, b)
    for a, b in zip(ph, ph2):
        for name in oh.state.get(a, {}):
            assert torch.equal(oh.state[a][name], oh2.state[b][name]), name


@pytest.mark.parametrize('amsgrad', [True, False])
def test_fused_adam_cross_loading(amsgrad):
    """10 steps with one optimiser, its state_dict into the other kind, 10 more: still inside the gate, either way round."""
    init = _refiner_params(SMALL)
    grads = _grads(init, 20)
    ref = _optimise('ref64', init, grads, amsgrad)
    t32 = _optimise('torch32', init, grads, amsgrad)
    for first, second in (('hip', 'torch32'), ('torch32', 'hip')):
        p1, o1, s1 = _optimise(first, init, grads[:10], amsgrad)
        mid = [p.detach().cpu() for p in p1]
        got = _optimise(second, mid, grads[10:], amsgrad, state=(o1.state_dict(), s1.state_dict()))
        assert got[1].param_groups[0]['lr'] == pytest.approx(1e-5)
        _gate_optimiser(got, ref, t32, '%s -> %s' % (first, second))


# ---------------------------------------------------------------------------------------------------------------------------------
# 8. - 10. the whole step
# ---------------------------------------------------------------------------------------------------------------------------------
def _trainer_setup(tmp_path, n=2):
    from frtm_vos_amd.evaluate import Parameters
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    from frtm_vos_amd.model.seg_network import SegNetwork
    from frtm_vos_amd.model.training_model import SampleSpec
    P = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18')
    P.disc_params.update(memory_size=20, init_iters=(3, 5), update_iters=(3,), c_channels=32)
    ext = ResnetFeatureExtractor('resnet18').to(DEV)
    chans = {L: c for L, c in ext.get_out_channels().items() if L in P.refnet_params.layers}
    torch.manual_seed(1)
    init = SegNetwork(1, 64, chans, True).to(DEV)
    seqs = [SyntheticSequence('s%d' % k, 3, (128, 160), 1, seed=30 + k) for k in range(n)]
    images = [torch.stack([s.images[t] for s in seqs]) for t in range(3)]
    labels = [torch.stack([(s.gt[t] == 1).to(torch.uint8) for s in seqs]) for t in range(3)]
    meta = [SampleSpec('s%d' % k, 1, ['00000', '00001', '00002'], 0).encoded() for k in range(n)]
    return P, ext, init, (images, labels, meta)


def _trainer_model(P, ext, refiner, cache, **kw):
    from frtm_vos_amd.model.augmenter import ImageAugmenter
    from frtm_vos_amd.model.training_model import TrainerModel
    return TrainerModel(ImageAugmenter(P.aug_params), ext, P.disc_params, refiner, batch_size=2, tmodel_cache=cache, device=DEV, **kw)


def test_step_has_no_framework_compute_and_one_read_back(tmp_path, monkeypatch):
    """Reads are counted through Tensor.item / .tolist / .cpu / .__float__ on CUDA tensors (the implementation uses one .tolist())."""
    from frtm_vos_amd.lib.fused_adam import FusedAdam
    P, ext, init, batch = _trainer_setup(tmp_path)
    cache = dict(path=tmp_path / 'cache', enable=True, read_only=False)
    refiner = copy.deepcopy(init)
    m = _trainer_model(P, ext, refiner, cache, refiner_backend='hip', loss_backend='hip')
    __import__('numpy').random.seed(0)
    assert m(*batch)['stats/fcache_hits'] == 0                            # fills the cache (the fit is not under test here)
    opt = FusedAdam(refiner.parameters(), lr=1e-3, weight_decay=1e-5, amsgrad=True)
    opt.zero_grad()

    def boom(*a, **k):
        raise AssertionError('framework compute in the training step')
    for name in ('binary_cross_entropy', 'binary_cross_entropy_with_logits', 'interpolate', 'conv2d', 'batch_norm', 'sigmoid'):
        monkeypatch.setattr(F, name, boom)
    for name in ['sigmoid', 'conv2d'] + [n for n in dir(torch) if n.startswith('_foreach_')]:
        monkeypatch.setattr(torch, name, boom)
    monkeypatch.setattr(torch.Tensor, 'sigmoid', boom)
    reads = []
    for name in ('item', 'tolist', 'cpu', '__float__'):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    before = [p.detach().clone() for p in refiner.parameters()]
    stats = m(*batch)
    in_forward = list(reads)
    opt.step()
    monkeypatch.undo()
    assert in_forward == ['tolist'], in_forward                          # once per call, not once per frame
    assert stats['stats/fcache_hits'] == 2 and 0 < stats['stats/loss'] < 5 and 0 <= stats['stats/accuracy'] <= 1
    assert all(p.grad is not None for p in refiner.parameters())
    assert sum(not torch.equal(a, b) for a, b in zip(before, refiner.parameters())) > 100
    # the same call with the torch loss reads back twice per frame of the sample set
    m2 = _trainer_model(P, ext, copy.deepcopy(init), cache, refiner_backend='hip', loss_backend='torch')
    s2 = m2(*batch)
    assert s2['stats/fcache_hits'] == 2


def test_whole_step_against_the_torch_tail(tmp_path):
    """Run A = HIP refiner pass + torch loss + torch.optim.Adam (the path before this change), run B = loss_backend='hip' + FusedAdam;
    the bars are those of test_refiner_train_gpu.py::test_trainer_model_hip_backend."""
    from frtm_vos_amd.lib.fused_adam import FusedAdam
    P, ext, init, batch = _trainer_setup(tmp_path)
    cache = dict(path=tmp_path / 'cache', enable=True, read_only=False)
    runs = {}
    for variant in ('A', 'B'):
        refiner = copy.deepcopy(init)
        m = _trainer_model(P, ext, refiner, cache, refiner_backend='hip', loss_backend='hip' if variant == 'B' else 'torch')
        __import__('numpy').random.seed(0)
        cls = FusedAdam if variant == 'B' else torch.optim.Adam
        opt = cls(refiner.parameters(), lr=1e-3, weight_decay=1e-5, amsgrad=True)
        losses, accs, grads = [], [], None
        for step in range(5):
            opt.zero_grad()
            st = m(*batch)
            losses.append(st['stats/loss'])
            accs.append(st['stats/accuracy'])
            if step == 0:
                grads = {k: p.grad.clone() for k, p in refiner.named_parameters()}
            opt.step()
        runs[variant] = (losses, accs, grads)
    (la, aa, ga), (lb, ab, gb) = runs['A'], runs['B']
    print('losses A %s\nlosses B %s\naccuracy A %s\naccuracy B %s' % (la, lb, aa, ab))
    assert abs(lb[0] - la[0]) <= 1e-4 * la[0]
    for k in ga:
        floor = 1e-3 * float(ga[k.replace('bias', 'weight')].abs().max()) if k.endswith('bblock.0.bias') else 0.0   # analytically zero
        assert _err(gb[k], ga[k]) <= max(1e-3 * float(ga[k].abs().max()), floor), k
    assert lb[-1] < lb[0] and la[-1] < la[0]
    assert abs(lb[-1] - la[-1]) <= 0.01 * la[-1]


def _driver(tmp_path, P, ext, init, dataset, cache, name, epochs):
    from frtm_vos_amd.lib.fused_adam import FusedAdam
    from frtm_vos_amd.lib.training import Trainer
    refiner = copy.deepcopy(init)
    m = _trainer_model(P, ext, refiner, cache, refiner_backend='hip', loss_backend='hip')
    opt = FusedAdam(refiner.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-5, amsgrad=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    tr = Trainer(name, m, opt, sched, dataset, tmp_path / 'ckpt', tmp_path / 'log', max_epochs=epochs, batch_size=2, save_interval=1)
    tr.train()
    return refiner, opt, tr


def test_trainer_resumes_bit_for_bit(tmp_path):
    import json
    from frtm_vos_amd.lib.training_datasets import SyntheticTrainingDataset
    P, ext, init, _ = _trainer_setup(tmp_path)

    def dataset():
        return SyntheticTrainingDataset(n_sequences=4, n_frames=6, size=(128, 160), seed=2)
    __import__('numpy').random.seed(0)
    cache = dict(path=tmp_path / 'cache', enable=True, read_only=False)
    _driver(tmp_path, P, ext, init, dataset(), cache, 'fill', 2)          # first pass: fits and stores every target model of epochs 1, 2
    cache = dict(cache, read_only=True)
    ref_a, opt_a, _ = _driver(tmp_path, P, ext, init, dataset(), cache, 'whole', 2)
    _driver(tmp_path, P, ext, init, dataset(), cache, 'split', 1)
    assert sorted(p.name for p in (tmp_path / 'ckpt' / 'split').iterdir()) == ['split_ep0001.pth']
    ref_b, opt_b, tr_b = _driver(tmp_path, P, ext, init, dataset(), cache, 'split', 2)    # fresh objects, state from the checkpoint
    assert tr_b.epoch == 2
    for name in ('whole', 'split'):
        lines = [json.loads(l) for l in open(tmp_path / 'log' / name / 'log.jsonl')]
        assert [l['epoch'] for l in lines] == [1, 2] and all(l['stats/fcache_hits'] == 2 for l in lines), lines
    sa, sb = ref_a.state_dict(), ref_b.state_dict()
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k                               # parameters and BatchNorm buffers
    assert any(k.endswith('running_mean') for k in sa)
    for pa, pb in zip(ref_a.parameters(), ref_b.parameters()):
        assert set(opt_a.state[pa]) == set(opt_b.state[pb]) == {'step', 'exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'}
        for name in opt_a.state[pa]:
            assert torch.equal(opt_a.state[pa][name], opt_b.state[pb][name]), name
    assert not torch.equal(next(ref_a.parameters()), next(init.parameters()))


def test_train_command_line(tmp_path):
    from frtm_vos_amd.evaluate import Parameters
    cmd = [sys.executable, '-m', 'frtm_vos_amd.train', 'cli', '--ftext', 'resnet18', '--dset', 'synthetic', '--epochs', '1', '--batch-size', '2',
           '--workspace', str(tmp_path), '--synthetic-sequences', '2', '--synthetic-size', '128x160', '--dev', DEV]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    file = tmp_path / 'checkpoints' / 'cli' / 'cli_ep0001.pth'
    assert file.exists() and (tmp_path / 'logs' / 'cli' / 'log.jsonl').exists()
    ck = torch.load(file, map_location='cpu')
    assert set(ck) == {'name', 'epoch', 'stats', 'model', 'optimizer', 'scheduler'} and ck['epoch'] == 1
    weights = ck['model']                                                 # evaluate.py: torch.load(file)['model']
    assert all(k.startswith('refiner.') for k in weights)
    P = Parameters(weights, fast=True, device=DEV)
    assert P.feature_extractor == 'resnet18' and P.in_channels == weights['refiner.TSE.layer4.reduce.0.weight'].shape[1] == 256
    tracker = P.get_model()                                               # loads the checkpoint into the inference model
    for k, v in tracker.refiner.state_dict().items():
        assert torch.equal(v.cpu(), weights['refiner.' + k]), k
