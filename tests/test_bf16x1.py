"""The bf16x1 trunk mode without a GPU: the ISA of csrc/conv_bf16x1.hip (its kernels, no scratch, no spills, bf16 MFMAs and the fp32 -> bf16
conversion in the K loop of every tile form, no fp32 MFMA), the C ABI, the argument check of frtm_backbone_set_bf16_pieces and the plumbing of the
precision from Parameters / the evaluate.py command line to the extractor."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
FORMS = ('k_conv1x1_bf16x1<128,64,64>', 'k_conv1x1_bf16x1<64,64,64>')        # frtm_conv_desc.tile 1 and 2: Cout x pixels x K chunk
KERNELS = set(FORMS) | {'k_pack_weights_bf16x1'}
NEW_SYMBOLS = ('frtm_conv_bf16x1_launches', 'frtm_backbone_set_bf16_pieces')


def kernel_name(demangled):
    """'void (anonymous namespace)::k<64, 64>(ConvParams)' -> 'k<64,64>'."""
    s = demangled.replace('(anonymous namespace)::', '')
    s = re.sub(r'^void\s+', '', s)
    return s.split('(')[0].replace(' ', '')


@pytest.fixture(scope='module')
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'bf16x1.s')
        p = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                            os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'conv_bf16x1.hip')], capture_output=True, text=True, cwd=d)
        assert p.returncode == 0, p.stderr[-2000:]
        return open(out).read()


def _bodies(isa):
    """mangled kernel name -> its instructions (from the symbol's label to .Lfunc_end)."""
    out = {}
    for m in re.finditer(r'^(_Z\S+):[^\n]*$(.*?)^\.Lfunc_end', isa, flags=re.M | re.S):
        out[m.group(1)] = m.group(2)
    return out


def _demangle(names):
    filt = shutil.which('c++filt') or shutil.which('llvm-cxxfilt') or '/opt/rocm/llvm/bin/llvm-cxxfilt'
    assert os.path.exists(filt) or shutil.which(filt), 'c++filt not found'
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


@pytest.mark.parametrize('form', FORMS)
def test_k_loop_runs_on_bf16_mfma_only(isa, form):
    bodies = _bodies(isa)
    names = _demangle(list(bodies))
    body = next(b for m, b in bodies.items() if names[m] == form)
    assert not re.search(r'v_mfma_f32_\w+_f32\b', body), 'an fp32 MFMA in the bf16x1 kernel'
    # the K loop: the block that ends in the backward branch (two chunks of four k-steps per trip)
    loops = []
    for m in re.finditer(r'^(\.LBB\d+_\d+):', body, flags=re.M):
        lab = m.group(1)
        for j in re.finditer(r's_(?:cbranch_\w+|branch)\s+' + re.escape(lab) + r'\b', body[m.end():]):
            loops.append(body[m.end():m.end() + j.start()])
    assert loops, 'no loop found'
    loop = max(loops, key=lambda b: b.count('v_mfma'))
    frags = {FORMS[0]: 2, FORMS[1]: 1}[form]                    # 32 x 32 fragments per wave
    assert loop.count('v_mfma_f32_32x32x16_bf16') == 8 * frags, loop.count('v_mfma_f32_32x32x16_bf16')
    assert loop.count('v_cvt_pk_bf16_f32') >= 8                 # the activations are converted inside the loop
    assert 'buffer_load_dword' in loop                          # ... from fp32 loads issued inside the loop


def test_abi_declares_exports_and_binds_the_new_symbols():
    from frtm_vos_amd import _hip
    hdr = open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read()
    L = _hip.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _hip.SIGNATURES and hasattr(L, name), name
    assert re.search(r'#define\s+FRTM_WLAYOUT_BF16X1\s+6\b', hdr)
    assert 'FRTM_CONV_BF16X1_ELEMS' in hdr
    assert L.frtm_conv_bf16x1_launches() >= 0          # callable without a device
    from frtm_vos_amd import ops
    # FRTM_CONV_BF16X1_ELEMS: Cin x Mp bf16 values in floats, Mp = Cout rounded up to 128; always a multiple of 4 floats
    assert ops.bf16x1_elems(256, 64) == 64 * 256 // 2 and ops.bf16x1_elems(65, 48) == 48 * 128 // 2 and ops.bf16x1_elems(130, 16) == 16 * 256 // 2


def test_set_bf16_pieces_validates_without_a_device():
    from frtm_vos_amd import _hip
    L = _hip.lib()
    bb = ctypes.c_void_p()
    assert L.frtm_backbone_create(50, ctypes.byref(bb)) == 0
    try:
        g0 = L.frtm_backbone_generation(bb)
        for bad in (2, 4, -1):
            assert L.frtm_backbone_set_bf16_pieces(bb, bad) == -1, bad
            assert b'frtm_backbone_set_bf16_pieces' in L.frtm_last_error()
            assert L.frtm_backbone_generation(bb) == g0          # the mode is unchanged
        # no conv is loaded: nothing to pack, so the valid modes need no device either; the generation moves with every change of mode only
        for pieces, bumps in ((1, 1), (1, 1), (3, 2), (0, 3), (0, 3)):
            assert L.frtm_backbone_set_bf16_pieces(bb, pieces) == 0, pieces
            assert L.frtm_backbone_generation(bb) == g0 + bumps, (pieces, bumps)
        assert L.frtm_backbone_set_precision(bb, 2) == -1        # the older switch keeps accepting exactly 0 and 1
        assert L.frtm_backbone_set_precision(bb, 1) == 0 and L.frtm_backbone_generation(bb) == g0 + 4
        assert L.frtm_backbone_set_bf16_pieces(bb, 3) == 0 and L.frtm_backbone_generation(bb) == g0 + 4      # 3 pieces IS mode 1
    finally:
        L.frtm_backbone_destroy(bb)


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
    for argv, want in (([], 'fp32'), (['--trunk-precision', 'bf16x1'], 'bf16x1')):
        args = parse_args(['--model', 'm.pth', '--dset', 'dv2017val'] + argv)
        assert args.trunk_precision == want
        p = parameters_from_args(args, None)
        assert p.trunk_precision == want
        with pytest.raises(Stop):
            p.get_model()
        assert seen[-1] == want
    assert Parameters(None, trunk_precision='bf16x1').trunk_precision == 'bf16x1'
    with pytest.raises(SystemExit):
        parse_args(['--model', 'm.pth', '--dset', 'dv2017val', '--trunk-precision', 'bf16'])
    with pytest.raises(ValueError):
        Parameters(None, trunk_precision='bf16')


def test_extractor_precision_property_without_a_device():
    import inspect
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    assert str(inspect.signature(ResnetFeatureExtractor.__init__)) == "(self, name='resnet101', weights=None, seed=0, precision='fp32')"
    ext = ResnetFeatureExtractor('resnet18', seed=0)
    assert ext.precision == 'fp32'
    ext.precision = 'bf16x1'                          # no backbone handle yet: recorded, applied by upload()
    assert ext.precision == 'bf16x1'
    with pytest.raises(ValueError):
        ext.precision = 'bf16'
    assert ext.precision == 'bf16x1'
    ext.precision = 'bf16x3'
    assert ext.precision == 'bf16x3'
    assert ResnetFeatureExtractor('resnet18', seed=0, precision='bf16x1').precision == 'bf16x1'
    with pytest.raises(ValueError):
        ResnetFeatureExtractor('resnet18', precision='bf16')
