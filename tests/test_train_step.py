"""CPU tests of the training step's ends and the driver: the C ABI of csrc/train_step.hip, its ISA (no spills, no scratch, no atomics,
16-byte accesses), the refusals that need no GPU, FusedAdam's torch-compatible state, Trainer (lib/training.py) on a stub model and
SyntheticTrainingDataset (lib/training_datasets.py)."""
import inspect
import json
import os
import re
import subprocess
import tempfile

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
NEW_ENTRY_POINTS = ['frtm_bce_logits_workspace_bytes', 'frtm_bce_logits', 'frtm_scale_by', 'frtm_adam_chunk_elems', 'frtm_adam_amsgrad']
KERNELS = ['k_bce_logits', 'k_bce_final', 'k_scale_by', 'k_adam']


# ---- 1. ABI ----
def test_abi_has_the_train_step_entry_points():
    from frtm_vos_amd import _hip
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read(), flags=re.S)
    L = _hip.lib()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _hip.SIGNATURES, name
        assert hasattr(L, name), name
    assert L.frtm_adam_chunk_elems() % 4 == 0 and L.frtm_adam_chunk_elems() >= 256
    assert L.frtm_bce_logits_workspace_bytes(16, 480, 854) > 0 and L.frtm_bce_logits_workspace_bytes(0, 480, 854) == 0


# ---- 2. ISA ----
@pytest.fixture(scope='module')
def step_isa():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'train_step.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'train_step.hip')], check=True, capture_output=True, cwd=d)
        return open(out).read()


def _kernel_bodies(isa, kernel):
    """name -> instruction text of every instantiation of ``kernel``."""
    code = isa[:isa.index('amdhsa.kernels:')]
    out = {}
    for m in re.finditer(r'^(_Z%d%s\w*):.*\n' % (len(kernel), kernel), code, flags=re.M):
        end = code.index('.Lfunc_end', m.end())
        out[m.group(1)] = code[m.end():end]
    return out


@pytest.mark.parametrize('kernel', KERNELS)
def test_step_kernels_spill_nothing(step_isa, kernel):
    meta = step_isa[step_isa.index('amdhsa.kernels:'):]
    blocks = [b for b in meta.split('\n  - ') if re.search(r'\.name:\s+_Z%d%s[A-Z]' % (len(kernel), kernel), b)]
    assert blocks, kernel
    for b in blocks:
        assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', b).group(1)) == 0
        assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', b).group(1)) == 0
        assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', b).group(1)) == 0


def test_step_kernels_use_no_atomics_and_wide_accesses(step_isa):
    code = step_isa[:step_isa.index('amdhsa.kernels:')]
    assert 'global_atomic' not in code and 'buffer_atomic' not in code and 'ds_add_f32' not in code and 'flat_atomic' not in code
    assert 'scratch_' not in code
    adam, bce = _kernel_bodies(step_isa, 'k_adam'), _kernel_bodies(step_isa, 'k_bce_logits')
    assert len(adam) == 2 and len(bce) == 2                      # amsgrad on / off; uint8 / fp32 targets
    for name, body in list(adam.items()) + list(bce.items()):
        assert 'global_load_dwordx4' in body and 'global_store_dwordx4' in body, name
        assert 'flat_load' not in body and 'flat_store' not in body, name      # table pointers stay in the global address space


# ---- 3. refusals and defaults ----
def test_trainer_model_loss_backend_argument():
    from frtm_vos_amd.model.training_model import TrainerModel
    with pytest.raises(ValueError, match='loss_backend'):
        TrainerModel(None, None, dict(layer='layer4'), None, loss_backend='bogus')
    params = inspect.signature(TrainerModel).parameters
    assert params['refiner_backend'].default == 'torch' and params['loss_backend'].default == 'torch'
    assert list(params).index('loss_backend') == list(params).index('refiner_backend') + 1


def test_loss_refuses_cpu_tensors():
    from frtm_vos_amd import ops
    from frtm_vos_amd.model.train_loss import bce_logits_stats
    z, t = torch.randn(2, 1, 8, 12), torch.zeros(2, 1, 8, 12, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bce_logits_stats(z, t)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.bce_logits(z, t)


def test_fused_adam_refusals():
    from frtm_vos_amd.lib.fused_adam import FusedAdam
    p = torch.nn.Parameter(torch.zeros(5))
    with pytest.raises(ValueError, match='maximize'):
        FusedAdam([p], maximize=True)
    for flag in ('capturable', 'differentiable'):
        with pytest.raises(ValueError, match=flag):
            FusedAdam([p], **{flag: True})
    opt = FusedAdam([p], lr=1e-3, amsgrad=True)
    p.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        opt.step()
    assert float(p.detach().abs().max()) == 0.0 and len(opt.state) == 0       # refused before anything was touched
    calls = []
    p.grad = None
    assert opt.step(lambda: calls.append(torch.is_grad_enabled()) or 7) == 7 and calls == [True]


# ---- 4. state layout ----
def _params():
    g = torch.Generator().manual_seed(0)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((4, 3, 3, 3), (4,), (1,), (7, 5))]


def _layout(sd):
    return ({k: {n: (type(v).__name__, getattr(v, 'dtype', None), tuple(getattr(v, 'shape', ()))) for n, v in s.items()} for k, s in sd['state'].items()},
            [{k: v for k, v in g.items()} for g in sd['param_groups']])


@pytest.mark.parametrize('amsgrad', [True, False])
def test_fused_adam_state_dict_is_torch_adams(amsgrad):
    from frtm_vos_amd.lib.fused_adam import FusedAdam
    kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-5, amsgrad=amsgrad)
    ref, fused = torch.optim.Adam(_params(), **kw), FusedAdam(_params(), **kw)
    assert isinstance(fused, torch.optim.Adam)
    assert _layout(fused.state_dict()) == _layout(ref.state_dict())                 # before any step
    for p in ref.param_groups[0]['params'][:3]:                                       # the last parameter stays without a gradient
        p.grad = torch.ones_like(p)
    ref.step()
    ref.step()
    fused.load_state_dict(ref.state_dict())
    a, b = _layout(fused.state_dict()), _layout(ref.state_dict())
    assert a == b and set(a[0]) == {0, 1, 2}
    assert set(a[0][0]) == {'step', 'exp_avg', 'exp_avg_sq'} | ({'max_exp_avg_sq'} if amsgrad else set())
    for k, s in ref.state_dict()['state'].items():
        for n, v in s.items():
            assert torch.equal(fused.state_dict()['state'][k][n], v), (k, n)
    back = torch.optim.Adam(_params(), **kw)
    back.load_state_dict(fused.state_dict())
    assert _layout(back.state_dict()) == b


def test_step_lr_drives_fused_adam():
    from frtm_vos_amd.lib.fused_adam import FusedAdam
    opt = FusedAdam(_params(), lr=1e-3, amsgrad=True, weight_decay=1e-5)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=2, gamma=0.1)
    lrs = []
    for _ in range(5):
        opt.step()                          # no gradients: nothing to do, nothing refused
        sched.step()
        lrs.append(opt.param_groups[0]['lr'])
    assert lrs == pytest.approx([1e-3, 1e-4, 1e-4, 1e-5, 1e-5])
    assert sched.get_last_lr() == pytest.approx([1e-5])


# ---- 5. driver and data ----
class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(2))
        self.seen = []

    def forward(self, images, labels, meta):
        self.seen.append(list(meta))
        loss = (self.w ** 2).sum() * (1 + 0.01 * float(images[1].float().mean()))
        loss.backward()
        return {'stats/loss': float(loss.detach()), 'stats/accuracy': 0.5, 'stats/fcache_hits': len(meta)}


def _stub_trainer(tmp_path, dataset, epochs, **kw):
    from frtm_vos_amd.lib.training import Trainer
    model = _Stub()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    return Trainer('run', model, opt, sched, dataset, tmp_path / 'ckpt', tmp_path / 'log', max_epochs=epochs, batch_size=2, **kw), model, opt, sched


def _dataset(**kw):
    from frtm_vos_amd.lib.training_datasets import SyntheticTrainingDataset
    return SyntheticTrainingDataset(n_sequences=5, n_frames=6, size=(96, 128), seed=3, **kw)


def test_trainer_checkpoints_resume_and_log(tmp_path):
    tr, model, opt, sched = _stub_trainer(tmp_path, _dataset(), 4, save_interval=2)
    tr.train()
    files = sorted(p.name for p in (tmp_path / 'ckpt' / 'run').iterdir())
    assert files == ['run_ep0002.pth', 'run_ep0004.pth']                                # save_interval honoured
    ck = torch.load(tmp_path / 'ckpt' / 'run' / 'run_ep0002.pth')
    assert set(ck) == {'name', 'epoch', 'stats', 'model', 'optimizer', 'scheduler'}
    assert ck['name'] == 'run' and ck['epoch'] == 2 and set(ck['model']) == {'w'}
    assert type(ck['stats']) is dict and all(type(v) is float for v in ck['stats'].values())
    assert {'stats/loss', 'stats/accuracy', 'stats/lr', 'stats/fcache_hits'} <= set(ck['stats'])
    assert ck['stats']['stats/lr'] == pytest.approx(0.05)                                # the lr epoch 2 ran with
    lines = [json.loads(l) for l in open(tmp_path / 'log' / 'run' / 'log.jsonl')]
    assert [l['epoch'] for l in lines] == [1, 2, 3, 4] and all('stats/loss' in l for l in lines)
    # a second trainer resumes after the newest checkpoint, with the scheduler's lr restored, and has nothing left to do
    tr2, model2, opt2, sched2 = _stub_trainer(tmp_path, _dataset(), 4)
    assert tr2.epoch == 4 and torch.equal(model2.w, model.w)
    assert opt2.param_groups[0]['lr'] == pytest.approx(0.1 * 0.5 ** 4) and sched2.get_last_lr() == pytest.approx([0.1 * 0.5 ** 4])
    tr2.train()
    assert model2.seen == []
    # resuming from epoch 2 replays epochs 3 and 4 exactly: same batches in the same order, same weights
    (tmp_path / 'ckpt' / 'run' / 'run_ep0004.pth').unlink()
    tr3, model3, _, _ = _stub_trainer(tmp_path, _dataset(), 4, save_interval=2)
    assert tr3.epoch == 2
    tr3.train()
    assert model3.seen == model.seen[len(model.seen) // 2:] and torch.equal(model3.w, model.w)
    # load_latest=False starts over
    tr4, _, _, _ = _stub_trainer(tmp_path, _dataset(), 4, load_latest=False)
    assert tr4.epoch == 0


def test_synthetic_training_dataset_contract():
    from frtm_vos_amd.model.training_model import SampleSpec
    d = _dataset(epoch_repeats=2)
    assert len(d) == 5 * 2
    images, labels, meta = d[3]
    assert len(images) == len(labels) == 3
    assert all(i.dtype == torch.uint8 and tuple(i.shape) == (3, 96, 128) for i in images)
    assert all(l.dtype == torch.uint8 and tuple(l.shape) == (1, 96, 128) and int(l.max()) <= 1 for l in labels)
    for k in range(len(d)):
        assert int(d[k][1][0].sum()) >= d.MIN_PIXELS                                     # frame 0 shows the object
    spec = SampleSpec.from_encoded([meta])[0]
    assert spec.encoded() == meta and spec.frame0_id == spec.frames[0] and len(set(spec.frames)) == 3
    assert spec.seq_name in d.sequences and spec.obj_id == 1
    first = [s.encoded() for s in d.specs]
    d.set_epoch(1)
    second = [s.encoded() for s in d.specs]
    d.set_epoch(0)
    assert [s.encoded() for s in d.specs] == first and second != first
    assert [s.encoded() for s in _dataset(epoch_repeats=2).specs] == first               # a fresh instance draws the same
    assert len(_dataset(epoch_samples=2)) == 2
    batch = next(iter(torch.utils.data.DataLoader(d, batch_size=2)))
    assert tuple(batch[0][0].shape) == (2, 3, 96, 128) and tuple(batch[1][2].shape) == (2, 1, 96, 128) and len(batch[2]) == 2


def test_train_command_line_defaults():
    from frtm_vos_amd.train import parse_args
    a = parse_args(['session'])
    assert (a.name, a.ftext, a.dev, a.dset, a.batch_size) == ('session', 'resnet101', 'cuda:0', 'synthetic', 16)
    b = parse_args(['s', '--ftext', 'resnet18', '--epochs', '1', '--batch-size', '2', '--workspace', 'w'])
    assert (b.ftext, b.epochs, b.batch_size, b.workspace) == ('resnet18', 1, 2, 'w')
