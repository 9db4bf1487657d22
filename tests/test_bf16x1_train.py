"""The bf16x1 refiner training mode without a GPU: the ISA of csrc/conv_wgrad_bf16x1.hip (its kernels, no scratch, no spills, bf16 MFMAs and aligned
16-byte LDS reads, no fp32 MFMA, no atomics), the C ABI and the workspace plan, the routing rule, SegNetwork.train_precision, and the plumbing of the
two precision flags of the train.py command line to SegNetwork and ResnetFeatureExtractor."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
KERNELS = {'k_conv_wgrad_bf16x1', 'k_wgrad_bf16x1_reduce'}
NAMES = ('frtm_conv_wgrad_bf16x1_ws_elems', 'frtm_conv_wgrad_bf16x1', 'frtm_conv_wgrad_bf16x1_launches')
FT = {'layer5': 64, 'layer4': 48, 'layer3': 32, 'layer2': 16}


@pytest.fixture(scope='module')
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'conv_wgrad_bf16x1.s')
        p = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                            os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'conv_wgrad_bf16x1.hip')], capture_output=True, text=True, cwd=d)
        assert p.returncode == 0, p.stderr[-2000:]
        return open(out).read()


def _demangle(names):
    filt = shutil.which('c++filt') or shutil.which('llvm-cxxfilt') or '/opt/rocm/llvm/bin/llvm-cxxfilt'
    assert os.path.exists(filt) or shutil.which(filt), 'c++filt not found'
    res = subprocess.run([filt], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    return [re.sub(r'^void\s+', '', n.replace('(anonymous namespace)::', '')).split('(')[0].replace(' ', '') for n in res[:len(names)]]


def test_kernels_are_the_expected_ones_without_scratch_or_spills(isa):
    mangled = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', isa, flags=re.M)
    assert set(_demangle(mangled)) == KERNELS and len(mangled) == len(KERNELS)
    assert re.findall(r'\.private_segment_fixed_size:\s+(\d+)', isa) == ['0'] * len(KERNELS)
    assert re.findall(r'\.vgpr_spill_count:\s+(\d+)', isa) == ['0'] * len(KERNELS)
    assert set(re.findall(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', isa)) == {'0'}
    assert all(int(v) <= 64 * 1024 for v in re.findall(r'\.group_segment_fixed_size:\s+(\d+)', isa))


def test_products_run_on_bf16_mfma_from_aligned_lds_reads(isa):
    assert isa.count('v_mfma_f32_32x32x16_bf16') >= 2 * 10              # per 16-pixel step: nine taps and the ones column
    assert not re.search(r'v_mfma_f32_\w+_f32\b', isa), 'an fp32 MFMA in the bf16x1 kernel'
    assert not re.search(r'global_atomic|buffer_atomic|flat_atomic|ds_\w*(?:add|cmpst|wrxchg)', isa), 'an atomic in the bf16x1 kernel'
    assert 'v_cvt_pk_bf16_f32' in isa                                    # rounded to nearest even in registers
    assert isa.count('ds_read_b128') >= 10 and not re.search(r'ds_read_u16|ds_read_u8', isa)       # whole operands, never assembled from halves
    assert 'buffer_load_dword' in isa


def test_abi_declares_exports_and_binds_the_new_symbols():
    import ctypes
    from frtm_vos_amd import _hip
    hdr = open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read()
    L = _hip.lib()
    for name in NAMES:
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _hip.SIGNATURES and hasattr(L, name), name
    assert L.frtm_conv_wgrad_bf16x1_launches() >= 0                       # callable without a device
    assert _hip.SIGNATURES['frtm_conv_wgrad_bf16x1_ws_elems'][0] is ctypes.c_size_t
    assert len(_hip.SIGNATURES['frtm_conv_wgrad_bf16x1'][1]) == 12        # the arguments of frtm_conv_wgrad without k


def plan(B, cout, cin, h, w):
    tiles = B * ((h + 3) // 4) * ((w + 31) // 32)
    ct = ((cin + 31) // 32) * ((cout + 63) // 64)
    rounds = -(-tiles * ct // (256 * 32))
    tps = -(-tiles * ct // (256 * rounds))
    return tiles, tps, (tiles + tps - 1) // tps


@pytest.mark.parametrize('shape,splits', [((1, 1, 1, 3, 3), 1), ((1, 64, 64, 4, 32), 1), ((2, 65, 65, 9, 11), 6), ((16, 64, 64, 15, 27), 64),
                                          ((1, 64, 64, 2081, 9), 105), ((16, 64, 64, 120, 214), 125), ((16, 32, 64, 240, 428), 498), ((16, 65, 65, 120, 214), 125), ((16, 64, 65, 120, 214), 168)])
def test_workspace_covers_the_plan(shape, splits):
    """Two slabs (one per pair of waves) of Cout x (9 Cin + 1) floats per split; one split, many splits, a ragged last one."""
    from frtm_vos_amd import _hip
    B, cout, cin, h, w = shape
    tiles, tps, nsplit = plan(*shape)
    assert nsplit == splits and 1 <= tps <= 32 and (nsplit - 1) * tps < tiles <= nsplit * tps
    assert _hip.lib().frtm_conv_wgrad_bf16x1_ws_elems(*shape) == 2 * nsplit * cout * (9 * cin + 1)
    assert _hip.lib().frtm_conv_wgrad_bf16x1_ws_elems(0, cout, cin, h, w) == 0


def test_routing_rule_is_one_function_of_the_launch():
    from frtm_vos_amd import ops
    # a number of blocks routes by size alone; 0 routes everything
    assert ops.bf16x1_wgrad_launch(1, 1, 1, 1, 1, 0) and ops.bf16x1_wgrad_launch(4, 4, 7, 65, 64, 0)
    assert not ops.bf16x1_wgrad_launch(1, 8, 8, 64, 32, 2) and ops.bf16x1_wgrad_launch(2, 8, 8, 64, 32, 2)
    # the measured rule: only table pairs, each only from its table count on
    for (cin, cout), blocks in ops.BF16X1_WGRAD_ROUTES.items():
        assert ops.bf16x1_wgrad_launch(64, 240, 428, cin, cout)
        n = -(-blocks // ((cout + 31) // 32))                     # maps of 8x8 that give exactly the table's block count, or just above it
        assert ops.bf16x1_wgrad_launch(n, 8, 8, cin, cout) and not ops.bf16x1_wgrad_launch(n - 1, 8, 8, cin, cout)
    assert (7, 7) not in ops.BF16X1_WGRAD_ROUTES and not ops.bf16x1_wgrad_launch(16, 120, 214, 7, 7)
    assert not ops.bf16x1_wgrad_launch(1 << 20, 240, 428, 7, 7)
    # the forward table keeps its entries
    for pair, blocks in {(64, 64): 896, (65, 65): 5376, (65, 64): 12960, (64, 65): 9720, (64, 32): 25920}.items():
        assert ops.BF16X1_3X3_ROUTES[pair] == blocks


def test_train_precision_property_without_a_device():
    from frtm_vos_amd.model.seg_network import SegNetwork
    net = SegNetwork(1, 64, dict(FT), use_bn=True)
    assert net.train_precision == 'fp32' and net.precision == 'fp32' and net.bf16_min_blocks is None
    net._pack_key, net._graphs = ('kept',), {'kept': 1}
    net.train_precision = 'bf16x1'
    assert net.train_precision == 'bf16x1' and net.precision == 'fp32' and net._pack_key == ('kept',) and net._graphs == {'kept': 1}
    with pytest.raises(ValueError):
        net.train_precision = 'bf16'
    with pytest.raises(ValueError):
        net.train_precision = 'bf16x3'
    assert net.train_precision == 'bf16x1'
    net.precision = 'bf16x1'                                          # the inference switch leaves the training one alone, and the reverse
    net.train_precision = 'fp32'
    assert net.train_precision == 'fp32' and net.precision == 'bf16x1'
    both = SegNetwork(1, 64, dict(FT), train_precision='bf16x1')
    assert both.train_precision == 'bf16x1' and both.precision == 'fp32'
    with pytest.raises(ValueError):
        SegNetwork(1, 64, dict(FT), train_precision='bf16x3')


def test_wrapper_refuses_other_kernel_sizes_before_any_call():
    import torch
    from frtm_vos_amd import ops
    x = torch.zeros(1, 4, 5, 5)
    with pytest.raises(ValueError):
        ops.conv_wgrad(x, x, 1, bf16x1=True)


def test_parameters_and_command_line_reach_the_refiner_and_the_trunk(monkeypatch):
    from frtm_vos_amd import train
    from frtm_vos_amd.model import feature_extractor, seg_network, training_model
    assert train.ModelParameters('n').refiner_precision == 'fp32' and train.ModelParameters('n').trunk_precision == 'fp32'
    made = []

    class Stop(Exception):
        pass

    class FakeExtractor:
        def __init__(self, name, **kw):
            made.append(('trunk', kw.get('precision', 'fp32')))

        def to(self, device):
            return self

        def get_out_channels(self):
            return dict(FT, layer1=8)

    real = seg_network.SegNetwork

    def fake_refiner(*a, **kw):
        net = real(*a, **kw)
        made.append(('refiner', net))
        return net

    def fake_trainer(augmenter, extractor, disc_params, refiner, **kw):
        raise Stop
    monkeypatch.setattr(feature_extractor, 'ResnetFeatureExtractor', FakeExtractor)
    monkeypatch.setattr(seg_network, 'SegNetwork', fake_refiner)
    monkeypatch.setattr(training_model, 'TrainerModel', fake_trainer)
    for argv, trunk, refiner in (([], 'fp32', 'fp32'), (['--refiner-precision', 'bf16x1'], 'fp32', 'bf16x1'),
                                 (['--trunk-precision', 'bf16x1'], 'bf16x1', 'fp32'),
                                 (['--trunk-precision', 'bf16x3', '--refiner-precision', 'bf16x1'], 'bf16x3', 'bf16x1')):
        args = train.parse_args(['name', '--dev', 'cpu'] + argv)
        assert (args.trunk_precision, args.refiner_precision) == (trunk, refiner)
        p = train.ModelParameters(args.name, device=args.dev, trunk_precision=args.trunk_precision, refiner_precision=args.refiner_precision)
        del made[:]
        with pytest.raises(Stop):
            p.get_model()
        assert made[0] == ('trunk', trunk)
        net = made[1][1]
        assert isinstance(net, real) and net.train_precision == refiner and net.precision == 'fp32'
    for bad in (['--refiner-precision', 'bf16'], ['--refiner-precision', 'bf16x3'], ['--trunk-precision', 'bf16']):
        with pytest.raises(SystemExit):
            train.parse_args(['name'] + bad)
    with pytest.raises(ValueError):
        train.ModelParameters('n', refiner_precision='bf16x3')
    with pytest.raises(ValueError):
        train.ModelParameters('n', trunk_precision='bf16')


def test_main_passes_both_flags_on(monkeypatch):
    from frtm_vos_amd import train
    seen = {}

    class Stop(Exception):
        pass

    class FakeParameters:
        def __init__(self, name, **kw):
            seen.update(kw)

        def get_model(self):
            raise Stop
    from frtm_vos_amd.lib import training_datasets
    monkeypatch.setattr(train, 'ModelParameters', FakeParameters)
    monkeypatch.setattr(training_datasets, 'SyntheticTrainingDataset', lambda **kw: None)      # (main builds the sample set first)
    with pytest.raises(Stop):
        train.main(['name', '--dev', 'cpu', '--refiner-precision', 'bf16x1', '--trunk-precision', 'bf16x1'])
    assert seen['refiner_precision'] == 'bf16x1' and seen['trunk_precision'] == 'bf16x1'
