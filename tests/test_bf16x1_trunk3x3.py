"""The bf16x1_3x3 trunk mode without a GPU: the ISA of csrc/conv3x3s2_bf16x1.hip (its kernels, no scratch, no spills, registers and LDS within the two
workgroups per CU its header claims, bf16 MFMAs and the fp32 -> bf16 conversion in the K loop of both tile forms, no fp32 MFMA, no atomic), the C ABI,
the argument check of frtm_backbone_set_bf16x1_3x3 and the plumbing of the precision from Parameters / the evaluate.py and train.py command lines to
the extractor."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
FORMS = ('k_conv3x3s2_bf16x1<2>', 'k_conv3x3s2_bf16x1<3>')        # frtm_conv_desc.tile 1 and 2: 64 and 96 output channels per workgroup
NEW_SYMBOLS = ('frtm_conv_bf16x1_3x3s2_launches', 'frtm_backbone_set_bf16x1_3x3')
MODES = ('fp32', 'bf16x3', 'bf16x1', 'bf16x1_3x3')
FT = {'layer5': 64, 'layer4': 48, 'layer3': 32, 'layer2': 16}


def kernel_name(demangled):
    """'void (anonymous namespace)::k<3>(ConvParams)' -> 'k<3>'."""
    s = demangled.replace('(anonymous namespace)::', '')
    s = re.sub(r'^void\s+', '', s)
    return s.split('(')[0].replace(' ', '')


@pytest.fixture(scope='module')
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'conv3x3s2_bf16x1.s')
        p = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                            os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'conv3x3s2_bf16x1.hip')], capture_output=True, text=True, cwd=d)
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
    assert set(_demangle(mangled).values()) == set(FORMS) and len(mangled) == len(FORMS)      # (the weight image is packed by conv3x3_bf16x1.hip's kernel)


def test_no_scratch_no_spills_and_two_workgroups_per_cu(isa):
    assert re.findall(r'\.private_segment_fixed_size:\s+(\d+)', isa) == ['0'] * len(FORMS)
    assert set(re.findall(r'\.vgpr_spill_count:\s+(\d+)', isa)) == {'0'}
    assert set(re.findall(r'\.sgpr_spill_count:\s+(\d+)', isa)) == {'0'}
    assert set(re.findall(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', isa)) == {'0'}
    # the header's two workgroups per CU: at most 256 registers per lane (AGPRs included) and half the CU's 160 KB of LDS
    vg, ag = re.findall(r'\.vgpr_count:\s+(\d+)', isa), re.findall(r'\.agpr_count:\s+(\d+)', isa)
    assert len(vg) == len(FORMS) and all(int(v) <= 256 for v in vg) and all(int(a) == 0 or int(a) <= 256 for a in ag)
    lds = [int(v) for v in re.findall(r'\.group_segment_fixed_size:\s+(\d+)', isa)]
    assert len(lds) == len(FORMS) and all(v <= 80 * 1024 for v in lds)
    # one stage of the 17 x 65 patch in two 8-channel groups and one of the 18 x BM weight slices, 16 bytes each
    assert sorted(lds) == [(2 * 17 * 65 + 18 * bm) * 16 for bm in (64, 96)]


@pytest.mark.parametrize('form', FORMS)
def test_k_loop_runs_on_bf16_mfma_only(isa, form):
    bodies = _bodies(isa)
    names = _demangle(list(bodies))
    body = next(b for m, b in bodies.items() if names[m] == form)
    assert not re.search(r'v_mfma_f32_\w+_f32\b', body), 'an fp32 MFMA in the bf16x1 kernel'
    assert not re.search(r'global_atomic|buffer_atomic|ds_\w*(?:add|cmpst|wrxchg)', body), 'an atomic in the bf16x1 kernel'
    # the K loop: the block that ends in the backward branch (one chunk of 16 channels: nine k-steps, one per tap)
    loops = []
    for m in re.finditer(r'^(\.LBB\d+_\d+):', body, flags=re.M):
        lab = m.group(1)
        for j in re.finditer(r's_(?:cbranch_\w+|branch)\s+' + re.escape(lab) + r'\b', body[m.end():]):
            loops.append(body[m.end():m.end() + j.start()])
    assert loops, 'no loop found'
    loop = max(loops, key=lambda b: b.count('v_mfma'))
    frags = {FORMS[0]: 2, FORMS[1]: 3}[form] * 2                # 32 x 32 fragments per wave: channels x two output rows
    assert loop.count('v_mfma_f32_32x32x16_bf16') == 9 * frags, loop.count('v_mfma_f32_32x32x16_bf16')
    assert loop.count('v_cvt_pk_bf16_f32') >= 8                 # the activations are converted inside the loop
    assert 'buffer_load_dword' in loop                          # ... from fp32 loads issued inside the loop
    assert 's_barrier' in loop
    assert 'ds_read_b128' in loop or 'ds_load_b128' in loop     # 16-byte fragment reads


def test_abi_declares_exports_and_binds_the_new_symbols():
    from frtm_vos_amd import _hip, build
    hdr = open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read()
    L = _hip.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _hip.SIGNATURES and hasattr(L, name), name
    assert re.search(r'#define\s+FRTM_WLAYOUT_BF16X1_3X3_S2\s+8\b', hdr) and re.search(r'#define\s+FRTM_WLAYOUT_BF16X1_3X3\s+7\b', hdr)
    assert L.frtm_conv_bf16x1_3x3s2_launches() >= 0          # callable without a device
    assert 'conv3x3s2_bf16x1.hip' in build.SOURCES


def test_set_bf16x1_3x3_validates_without_a_device():
    from frtm_vos_amd import _hip
    L = _hip.lib()
    bb = ctypes.c_void_p()
    assert L.frtm_backbone_create(18, ctypes.byref(bb)) == 0
    try:
        g0 = L.frtm_backbone_generation(bb)
        for bad in (2, -1, 3):
            assert L.frtm_backbone_set_bf16x1_3x3(bb, bad) == -1, bad
            assert b'frtm_backbone_set_bf16x1_3x3' in L.frtm_last_error()
            assert L.frtm_backbone_generation(bb) == g0          # the state is unchanged
        # no conv is loaded: nothing to pack, so the switch needs no device; the generation moves only when the flag's value changes
        for on, bumps in ((0, 0), (1, 1), (1, 1), (0, 2), (0, 2)):
            assert L.frtm_backbone_set_bf16x1_3x3(bb, on) == 0, on
            assert L.frtm_backbone_generation(bb) == g0 + bumps, (on, bumps)
        # the flag is stored independently of the pieces mode, which keeps its own values and bumps
        assert L.frtm_backbone_set_bf16x1_3x3(bb, 1) == 0 and L.frtm_backbone_generation(bb) == g0 + 3
        for pieces, bumps in ((1, 4), (1, 4), (3, 5), (0, 6)):
            assert L.frtm_backbone_set_bf16_pieces(bb, pieces) == 0 and L.frtm_backbone_generation(bb) == g0 + bumps, pieces
        assert L.frtm_backbone_set_bf16_pieces(bb, 2) == -1 and L.frtm_backbone_generation(bb) == g0 + 6
        assert L.frtm_backbone_set_bf16x1_3x3(bb, 1) == 0 and L.frtm_backbone_generation(bb) == g0 + 6        # still on: no change
        assert L.frtm_backbone_set_bf16x1_3x3(None, 1) == -1
    finally:
        L.frtm_backbone_destroy(bb)


def test_extractor_precision_property_round_trips_without_a_device():
    import inspect
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    assert str(inspect.signature(ResnetFeatureExtractor.__init__)) == "(self, name='resnet101', weights=None, seed=0, precision='fp32')"
    ext = ResnetFeatureExtractor('resnet18', seed=0)
    assert ext.precision == 'fp32'
    for mode in MODES[1:] + MODES:                    # no backbone handle yet: recorded, applied by upload()
        ext.precision = mode
        assert ext.precision == mode
    ext.precision = 'bf16x1_3x3'
    for bad in ('bf16', 'bf16x3_3x3', 'bf16x1_3X3', None):
        with pytest.raises(ValueError):
            ext.precision = bad
        assert ext.precision == 'bf16x1_3x3'
    assert ResnetFeatureExtractor('resnet18', seed=0, precision='bf16x1_3x3').precision == 'bf16x1_3x3'
    with pytest.raises(ValueError):
        ResnetFeatureExtractor('resnet18', precision='bf16x1_3')


def test_extractor_sets_pieces_and_flag_per_mode(monkeypatch):
    """With a handle, every mode sets the pieces AND the flag: bf16x1_3x3 = (1, on), every other mode (its pieces, off)."""
    from frtm_vos_amd.model import feature_extractor as FE
    calls = []
    monkeypatch.setattr(FE.H, 'call_nostream', lambda name, handle, *a: calls.append((name,) + a))
    ext = FE.ResnetFeatureExtractor('resnet18', seed=0)
    for mode, pieces in (('bf16x1_3x3', 1), ('bf16x1', 1), ('bf16x3', 3), ('bf16x1_3x3', 1), ('fp32', 0)):
        del calls[:]
        ext._apply_precision(mode)
        assert calls == [('frtm_backbone_set_bf16_pieces', pieces), ('frtm_backbone_set_bf16x1_3x3', int(mode == 'bf16x1_3x3'))], (mode, calls)


def test_parameters_and_evaluate_command_line_reach_the_extractor(monkeypatch):
    from frtm_vos_amd import evaluate
    from frtm_vos_amd.evaluate import Parameters, parameters_from_args, parse_args
    from frtm_vos_amd.model import feature_extractor as FE
    assert Parameters(None).trunk_precision == 'fp32'
    seen = []

    class Stop(Exception):
        pass

    def fake_init(self, name, weights=None, seed=0, precision='fp32'):
        seen.append((name, precision))
        raise Stop
    monkeypatch.setattr(FE.ResnetFeatureExtractor, '__init__', fake_init)
    monkeypatch.setattr(evaluate, 'ResnetFeatureExtractor', FE.ResnetFeatureExtractor)
    for argv, want in (([], 'fp32'), (['--trunk-precision', 'bf16x1_3x3'], 'bf16x1_3x3')):
        args = parse_args(['--model', 'm.pth', '--dset', 'dv2017val'] + argv)
        assert args.trunk_precision == want
        p = parameters_from_args(args, None)
        assert p.trunk_precision == want
        with pytest.raises(Stop):
            p.get_model()
        assert seen[-1][1] == want
    p = Parameters(None, fast=True, feature_extractor='resnet18', trunk_precision='bf16x1_3x3')
    assert p.trunk_precision == 'bf16x1_3x3'
    with pytest.raises(Stop):
        p.get_model()
    assert seen[-1] == ('resnet18', 'bf16x1_3x3')
    for bad in ('bf16x1_3', 'bf16x3_3x3'):
        with pytest.raises(SystemExit):
            parse_args(['--model', 'm.pth', '--dset', 'dv2017val', '--trunk-precision', bad])
        with pytest.raises(ValueError):
            Parameters(None, trunk_precision=bad)


def test_train_parameters_and_command_line_reach_the_extractor(monkeypatch):
    from frtm_vos_amd import train
    from frtm_vos_amd.model import feature_extractor, training_model
    made = []

    class Stop(Exception):
        pass

    class FakeExtractor:
        def __init__(self, name, **kw):
            made.append(kw.get('precision', 'fp32'))

        def to(self, device):
            return self

        def get_out_channels(self):
            return dict(FT, layer1=8)

    def fake_trainer(augmenter, extractor, disc_params, refiner, **kw):
        raise Stop
    monkeypatch.setattr(feature_extractor, 'ResnetFeatureExtractor', FakeExtractor)
    monkeypatch.setattr(training_model, 'TrainerModel', fake_trainer)
    for argv, want in (([], 'fp32'), (['--trunk-precision', 'bf16x1_3x3'], 'bf16x1_3x3')):
        args = train.parse_args(['name', '--dev', 'cpu'] + argv)
        assert args.trunk_precision == want
        p = train.ModelParameters(args.name, device=args.dev, trunk_precision=args.trunk_precision)
        assert p.trunk_precision == want
        with pytest.raises(Stop):
            p.get_model()
        assert made[-1] == want
    with pytest.raises(SystemExit):
        train.parse_args(['name', '--trunk-precision', 'bf16x1_3'])
    with pytest.raises(ValueError):
        train.ModelParameters('n', trunk_precision='bf16x1_3')
    # main() hands the flag on
    seen = {}

    class FakeParameters:
        def __init__(self, name, **kw):
            seen.update(kw)

        def get_model(self):
            raise Stop
    from frtm_vos_amd.lib import training_datasets
    monkeypatch.setattr(train, 'ModelParameters', FakeParameters)
    monkeypatch.setattr(training_datasets, 'SyntheticTrainingDataset', lambda **kw: None)      # (main builds the sample set first)
    with pytest.raises(Stop):
        train.main(['name', '--dev', 'cpu', '--trunk-precision', 'bf16x1_3x3'])
    assert seen['trunk_precision'] == 'bf16x1_3x3'
