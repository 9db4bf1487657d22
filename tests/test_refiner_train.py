"""CPU tests of the refiner's HIP training pass (SegNetwork.forward_train, TrainerModel(refiner_backend=)): the refusals that need no GPU,
and the register / scratch budget and atomic-free form of csrc/refiner_train.hip."""
import os
import re
import subprocess
import tempfile
from collections import OrderedDict

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
CHANS = OrderedDict(layer5=32, layer4=16, layer3=8, layer2=8)
KERNELS = ['k_conv_wgrad', 'k_conv_wgrad_reduce', 'k_bn_stats_part', 'k_bn_stats_final', 'k_bn_apply_relu', 'k_bn_bwd_part', 'k_bn_bwd_apply',
           'k_relu_bwd', 'k_pyrup2x_bwd_axis', 'k_bilinear_bwd_axis', 'k_cab_bwd_reduce', 'k_cab_gate_bwd', 'k_cab_bwd_shallow', 'k_add_plane',
           'k_shift9']


def _inputs():
    feats = {L: torch.randn(1, c, 3 * 2 ** i, 5 * 2 ** i) for i, (L, c) in enumerate(CHANS.items())}
    return torch.randn(1, 1, 6, 10), feats


def test_forward_train_refuses_cpu_tensors():
    from frtm_vos_amd.model.seg_network import SegNetwork
    net = SegNetwork(1, 8, CHANS, True)
    scores, feats = _inputs()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net.forward_train(scores, feats, (48, 80))


def test_forward_train_refuses_bicubic_head():
    from frtm_vos_amd.model.seg_network import SegNetwork
    net = SegNetwork(1, 8, CHANS, True, upsampler='bicubic')
    scores, feats = _inputs()
    with pytest.raises(NotImplementedError, match='Upsampler.*forward_torch'):
        net.forward_train(scores, feats, (48, 80))


def test_trainer_model_backend_argument():
    from frtm_vos_amd.model.training_model import TrainerModel
    with pytest.raises(ValueError, match='refiner_backend'):
        TrainerModel(None, None, dict(layer='layer4'), None, refiner_backend='bogus')
    import inspect
    assert inspect.signature(TrainerModel).parameters['refiner_backend'].default == 'torch'


@pytest.fixture(scope='module')
def train_isa():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'refiner_train.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'refiner_train.hip')], check=True, capture_output=True, cwd=d)
        return open(out).read()


@pytest.mark.parametrize('kernel', KERNELS)
def test_train_kernels_spill_nothing(train_isa, kernel):
    meta = train_isa[train_isa.index('amdhsa.kernels:'):]
    blocks = [b for b in meta.split('\n  - ') if re.search(r'\.name:\s+_Z%d%s[A-Z]' % (len(kernel), kernel), b)]
    assert blocks, kernel
    for b in blocks:
        assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', b).group(1)) == 0
        assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', b).group(1)) == 0
        assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', b).group(1)) == 0


def test_train_kernels_use_no_atomics_and_mfma_wgrad(train_isa):
    """Determinism is structural: no float atomics anywhere; the weight gradient runs on the fp32 MFMA."""
    code = train_isa[:train_isa.index('amdhsa.kernels:')]
    assert 'global_atomic' not in code and 'buffer_atomic' not in code and 'ds_add_f32' not in code
    assert 'v_mfma_f32_32x32x2_f32' in code
