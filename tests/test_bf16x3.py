"""The bf16x3 trunk mode without a GPU: the ISA of csrc/conv_bf16x3.hip (its kernels, no scratch, no spills, bf16 MFMAs and no fp32 MFMA in the K
loop) and the plumbing of the precision from Parameters / the evaluate.py command line to the extractor."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from test_conv_forms import kernel_name

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
KERNELS = {'k_conv1x1_bf16x3', 'k_pack_weights_bf16x3'}


@pytest.fixture(scope='module')
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'bf16x3.s')
        p = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                            os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'conv_bf16x3.hip')], capture_output=True, text=True, cwd=d)
        assert p.returncode == 0, p.stderr[-2000:]
        return open(out).read()


def _bodies(isa):
    """mangled kernel name -> its instructions (from the symbol's label to .Lfunc_end)."""
    out = {}
    for m in re.finditer(r'^(_Z\S+):[^\n]*$(.*?)^\.Lfunc_end', isa, flags=re.M | re.S):
        out[m.group(1)] = m.group(2)
    return out


def _demangle(names):
    filt = shutil.which('c++filt') or shutil.which('llvm-cxxfilt')
    assert filt, 'c++filt not found'
    res = subprocess.run([filt], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    return dict(zip(names, (kernel_name(n) for n in res)))


def test_kernels_are_exactly_the_expected_ones(isa):
    mangled = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', isa, flags=re.M)
    assert set(_demangle(mangled).values()) == KERNELS and len(mangled) == len(KERNELS)


def test_no_scratch_no_spills(isa):
    assert re.findall(r'\.private_segment_fixed_size:\s+(\d+)', isa) == ['0'] * len(KERNELS)
    assert set(re.findall(r'\.vgpr_spill_count:\s+(\d+)', isa)) == {'0'}
    assert set(re.findall(r'\.sgpr_spill_count:\s+(\d+)', isa)) == {'0'}
    assert set(re.findall(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', isa)) == {'0'}


def test_k_loop_runs_on_bf16_mfma_only(isa):
    bodies = _bodies(isa)
    names = _demangle(list(bodies))
    body = next(b for m, b in bodies.items() if names[m] == 'k_conv1x1_bf16x3')
    assert not re.search(r'v_mfma_f32_\w+_f32\b', body), 'an fp32 MFMA in the bf16x3 kernel'
    # the K loop: the block that ends in the backward branch; six piece products x 2 x 2 fragments per chunk of 16
    loops = []
    for m in re.finditer(r'^(\.LBB\d+_\d+):', body, flags=re.M):
        lab = m.group(1)
        j = re.search(r's_(?:cbranch_\w+|branch)\s+' + re.escape(lab) + r'\b', body[m.end():])
        if j:
            loops.append(body[m.end():m.end() + j.start()])
    assert loops, 'no loop found'
    loop = max(loops, key=lambda b: b.count('v_mfma'))
    assert loop.count('v_mfma_f32_32x32x16_bf16') == 24, loop.count('v_mfma_f32_32x32x16_bf16')
    assert loop.count('v_cvt_pk_bf16_f32') >= 12                     # the activations are split inside the loop
    assert 'v_mfma_f32_16x16x4_f32' not in loop and 'v_mfma_f32_32x32x2_f32' not in loop


def test_parameters_and_command_line_reach_the_extractor(monkeypatch):
    from frtm_vos_amd import evaluate
    from frtm_vos_amd.evaluate import Parameters, parameters_from_args, parse_args
    from frtm_vos_amd.model import feature_extractor as FE
    assert Parameters(None).trunk_precision == 'fp32'
    seen = []

    class Stop(Exception):
        pass

    def fake_init(self, name, weights=None, seed=0, precision='fp32'):
        seen.append(precision)
        raise Stop
    monkeypatch.setattr(FE.ResnetFeatureExtractor, '__init__', fake_init)
    monkeypatch.setattr(evaluate, 'ResnetFeatureExtractor', FE.ResnetFeatureExtractor)
    for argv, want in (([], 'fp32'), (['--trunk-precision', 'bf16x3'], 'bf16x3'), (['--trunk-precision', 'fp32'], 'fp32')):
        args = parse_args(['--model', 'm.pth', '--dset', 'dv2017val'] + argv)
        assert args.trunk_precision == want
        p = parameters_from_args(args, None)
        assert p.trunk_precision == want
        with pytest.raises(Stop):
            p.get_model()
        assert seen[-1] == want
    with pytest.raises(SystemExit):
        parse_args(['--model', 'm.pth', '--dset', 'dv2017val', '--trunk-precision', 'bf16'])
    with pytest.raises(ValueError):
        Parameters(None, trunk_precision='tf32')


def test_extractor_precision_property_without_a_device():
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    ext = ResnetFeatureExtractor('resnet18', seed=0)
    assert ext.precision == 'fp32'
    ext.precision = 'bf16x3'                          # no backbone handle yet: recorded, applied by upload()
    assert ext.precision == 'bf16x3'
    with pytest.raises(ValueError):
        ext.precision = 'half'
    assert ext.precision == 'bf16x3'
    assert ResnetFeatureExtractor('resnet18', seed=0, precision='bf16x3').precision == 'bf16x3'
    with pytest.raises(ValueError):
        ResnetFeatureExtractor('resnet18', precision='fp16')
