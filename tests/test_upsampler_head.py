"""CPU tests of the bicubic refiner head (model/seg_network.py: Upsampler, the head of the reference's YouTube-VOS fork): the PyTorch
definition against fixture G19 (recorded from the fork by tools/make_golden_g19.py), the checkpoint layout shared with the compat head,
the driver options that select it, and the register / scratch budget of its two HIP kernels."""
import os
import re
import subprocess
import tempfile
import zlib
from collections import OrderedDict

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
T = torch.from_numpy
CHANS = OrderedDict(layer5=32, layer4=16, layer3=8, layer2=8)


def _keyed_state_dict(module):
    """oracle/make_golden.py: keyed_state_dict (weights seeded by the key NAME), restated without the reference harness."""
    sd = {}
    for k, v in module.state_dict().items():
        g = torch.Generator().manual_seed(zlib.crc32(k.encode()) & 0x7fffffff)
        if k.endswith('num_batches_tracked'):
            sd[k] = v.clone()
        elif k.endswith('running_var'):
            sd[k] = torch.rand(v.shape, generator=g) + 0.5
        elif v.dim() == 4:
            sd[k] = torch.randn(v.shape, generator=g) / (v.shape[1] * v.shape[2] * v.shape[3]) ** 0.5
        else:
            sd[k] = torch.randn(v.shape, generator=g) * 0.1 + (1.0 if k.endswith('.1.weight') else 0.0)
    return sd


def test_segnetwork_bicubic_head_g19(golden):
    """The batched refiner with upsampler='bicubic' (forward_torch on the CPU) == the fork's per-object refiner, same checkpoint keys."""
    from frtm_vos_amd.model.seg_network import SegNetwork, Upsampler
    g = golden('g19_upsampler')
    net = SegNetwork(1, 8, CHANS, True, upsampler='bicubic').eval()
    assert isinstance(net.project, Upsampler)
    assert len(net.state_dict()) == int(g['nkeys'])
    net.load_state_dict(_keyed_state_dict(net))
    for tag in ('A', 'B'):
        feats = {L: T(g['%s_ft_%s' % (tag, L)]) for L in CHANS}
        scores = T(g[tag + '_scores'])
        size = tuple(int(v) for v in g[tag + '_size'])
        with torch.no_grad():
            out = net(scores, feats, size)                   # all objects in one pass
        ref = T(g[tag + '_out'])
        assert out.shape == ref.shape == (scores.shape[0], 1) + size
        assert float((out - ref).abs().max()) < 2e-5, tag


def test_upsampler_equals_reference_upsampler(golden):
    from frtm_vos_amd.model.seg_network import Upsampler
    g = golden('g19_upsampler')
    up = Upsampler(16).eval()
    up.load_state_dict(_keyed_state_dict(up))
    with torch.no_grad():
        out = up(T(g['up_in']), tuple(int(v) for v in g['up_size']))
    assert out.shape == (1, 1, 40, 57)
    assert float((out - T(g['up_out'])).abs().max()) < 2e-5


def test_both_heads_share_the_checkpoint_layout():
    """A fork checkpoint loads into either head (strict), so only the head's type decides what runs."""
    from frtm_vos_amd.model.seg_network import BackwardCompatibleUpsampler, SegNetwork, Upsampler
    compat = SegNetwork(1, 8, CHANS, True)
    bicubic = SegNetwork(1, 8, CHANS, True, upsampler='bicubic')
    assert isinstance(compat.project, BackwardCompatibleUpsampler) and isinstance(bicubic.project, Upsampler)
    sc, sb = compat.state_dict(), bicubic.state_dict()
    assert list(sc) == list(sb)
    assert all(sc[k].shape == sb[k].shape for k in sc)
    bicubic.load_state_dict(sc)
    with pytest.raises(ValueError, match='upsampler'):
        SegNetwork(1, 8, CHANS, True, upsampler='bilinear')


def test_swapping_the_head_drops_packed_weights_and_graphs():
    from frtm_vos_amd.model.seg_network import SegNetwork, Upsampler
    net = SegNetwork(1, 8, CHANS, True)
    net._pack_key, net._graphs = ('stale',), {'k': None}
    net.project = Upsampler(8)
    assert net._pack_key is None and net._graphs == {}


def test_driver_selects_the_head():
    """--upsampler / --ytvos-fork reach SegNetwork through Parameters; the default command line keeps the compat head."""
    from frtm_vos_amd.evaluate import Parameters, parameters_from_args, parse_args
    from frtm_vos_amd.model.seg_network import BackwardCompatibleUpsampler, Upsampler
    base = ['--model', 'ck.pth', '--dset', 'yt2018val']
    chans = OrderedDict(layer5=2048, layer4=1024, layer3=512, layer2=256)
    a = parse_args(base)
    assert (a.upsampler, a.ytvos_solver, a.ytvos_merge) == ('compat', False, False)
    assert isinstance(parameters_from_args(a, None).make_refiner(chans).project, BackwardCompatibleUpsampler)
    a = parse_args(base + ['--ytvos-fork'])
    assert (a.upsampler, a.ytvos_solver, a.ytvos_merge) == ('bicubic', True, True)
    p = parameters_from_args(a, None)
    assert p.disc_params.fletcher_reeves and p.disc_params.CG_forgetting_rate is None
    assert isinstance(p.make_refiner(chans).project, Upsampler)
    assert parse_args(base + ['--upsampler', 'bicubic']).ytvos_merge is False
    assert Parameters(None, device='cpu').upsampler == 'compat'
    # same seeded default init for both heads: the parameters are drawn in the same order
    r0 = Parameters(None, device='cpu').make_refiner(chans)
    r1 = Parameters(None, device='cpu', upsampler='bicubic').make_refiner(chans)
    assert all(torch.equal(x, y) for x, y in zip(r0.state_dict().values(), r1.state_dict().values()))


@pytest.fixture(scope='module')
def refiner_isa():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'refiner.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'refiner_ops.hip')], check=True, capture_output=True, cwd=d)
        return open(out).read()


@pytest.mark.parametrize('kernel', ['k_bicubic_resize', 'k_project_tail_bicubic'])
def test_bicubic_kernels_spill_nothing(refiner_isa, kernel):
    """Neither kernel spills registers or uses a private (scratch) segment."""
    meta = refiner_isa[refiner_isa.index('amdhsa.kernels:'):]
    blocks = [b for b in meta.split('\n  - ') if re.search(r'\.name:\s+_Z%d%s[A-Z]' % (len(kernel), kernel), b)]
    assert len(blocks) == 1, kernel
    b = blocks[0]
    assert int(re.search(r'\.vgpr_spill_count:\s+(\d+)', b).group(1)) == 0
    assert int(re.search(r'\.sgpr_spill_count:\s+(\d+)', b).group(1)) == 0
    assert int(re.search(r'\.private_segment_fixed_size:\s+(\d+)', b).group(1)) == 0
