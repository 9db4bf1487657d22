"""The bf16x1 refiner mode without a GPU: the ISA of csrc/conv3x3_bf16x1.hip (its kernels, no scratch, no spills, bf16 MFMAs and the fp32 -> bf16
conversion in the K loop of every tile form, no fp32 MFMA), the C ABI, and the plumbing of the precision from Parameters / the evaluate.py command line
to SegNetwork."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
FORMS = ('k_conv3x3_bf16x1<2>', 'k_conv3x3_bf16x1<3>')        # frtm_conv_desc.tile 1 and 2: 32-row fragments per workgroup (64 and 96 output channels)
KERNELS = set(FORMS) | {'k_pack_weights_bf16x1_3x3'}
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
        out = os.path.join(d, 'conv3x3_bf16x1.s')
        p = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                            os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'conv3x3_bf16x1.hip')], capture_output=True, text=True, cwd=d)
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
    # two workgroups per CU: at most 256 registers per lane and half the CU's 160 KB of LDS
    assert all(int(v) <= 256 for v in re.findall(r'\.vgpr_count:\s+(\d+)', isa))
    assert all(int(v) <= 80 * 1024 for v in re.findall(r'\.group_segment_fixed_size:\s+(\d+)', isa))


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


def test_abi_declares_exports_and_binds_the_new_symbol():
    from frtm_vos_amd import _hip, ops
    hdr = open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read()
    L = _hip.lib()
    name = 'frtm_conv_bf16x1_3x3_launches'
    assert re.search(r'\b%s\s*\(' % name, hdr) and name in _hip.SIGNATURES and hasattr(L, name)
    assert L.frtm_conv_bf16x1_3x3_launches() >= 0          # callable without a device
    assert re.search(r'#define\s+FRTM_WLAYOUT_BF16X1_3X3\s+7\b', hdr) and re.search(r'#define\s+FRTM_WLAYOUT_BF16X1\s+6\b', hdr)
    assert re.search(r'#define\s+FRTM_BF16X1_3X3_TILE_64\s+1\b', hdr) and re.search(r'#define\s+FRTM_BF16X1_3X3_TILE_96\s+2\b', hdr)
    # FRTM_CONV_BF16X1_3X3_ELEMS, evaluated by the C preprocessor's own arithmetic (the macro's text as a Python expression), against ops
    m = re.search(r'#define\s+FRTM_CONV_BF16X1_3X3_ELEMS\(Cout, Cin\)\s+(.*)', hdr)
    assert m
    expr = m.group(1).replace('(size_t)', '').replace('/', '//')
    for cout, cin in ((64, 64), (65, 65), (32, 64), (1, 1), (80, 24)):
        want = eval(expr, {'Cout': cout, 'Cin': cin})
        assert ops.bf16x1_3x3_elems(cout, cin) == want, (cout, cin)
        assert want == 9 * ((cin + 15) // 16 * 16) * ((cout + 31) // 32 * 32) // 2 and want % 4 == 0
    assert ops.bf16x1_3x3_elems(65, 65) == 9 * 80 * 96 // 2


def test_routing_rule_is_one_function_of_the_launch():
    from frtm_vos_amd import ops
    # a number of blocks routes by size alone; 0 routes everything
    assert ops.bf16x1_3x3_launch(1, 1, 1, 1, 1, 0) and ops.bf16x1_3x3_launch(4, 4, 7, 65, 64, 0)
    assert not ops.bf16x1_3x3_launch(1, 8, 8, 64, 32, 2) and ops.bf16x1_3x3_launch(2, 8, 8, 64, 32, 2)
    # the measured rule never takes a launch that wino_launch refuses (nothing below that size was measured), and only measured channel pairs
    assert not ops.bf16x1_3x3_launch(1, 8, 8, 64, 64)
    for (cin, cout), blocks in ops.BF16X1_3X3_ROUTES.items():
        assert ops.bf16x1_3x3_launch(64, 240, 428, cin, cout) and ops.wino_launch(64, 240, 428, cout)
        n = -(-blocks // ((cout + 31) // 32))                     # maps of 8x8 that give exactly the table's block count, or just above it
        assert ops.bf16x1_3x3_launch(n, 8, 8, cin, cout) and not ops.bf16x1_3x3_launch(n - 1, 8, 8, cin, cout)
    assert not ops.bf16x1_3x3_launch(16, 120, 214, 7, 7)


def test_precision_property_without_a_device():
    from frtm_vos_amd.model.seg_network import SegNetwork
    net = SegNetwork(1, 64, dict(FT), use_bn=True)
    assert net.precision == 'fp32' and net.bf16_min_blocks is None
    net._pack_key, net._graphs = ('stale',), {'stale': 1}
    net.precision = 'bf16x1'
    assert net.precision == 'bf16x1' and net._pack_key is None and net._graphs == {}
    with pytest.raises(ValueError):
        net.precision = 'bf16'
    assert net.precision == 'bf16x1'
    net._pack_key, net._graphs = ('stale',), {'stale': 1}
    net.precision = 'fp32'
    assert net.precision == 'fp32' and net._pack_key is None and net._graphs == {}
    assert SegNetwork(1, 64, dict(FT), precision='bf16x1').precision == 'bf16x1'
    with pytest.raises(ValueError):
        SegNetwork(1, 64, dict(FT), precision='bf16x3')


def test_parameters_and_command_line_reach_the_refiner(monkeypatch):
    from frtm_vos_amd import evaluate
    from frtm_vos_amd.evaluate import Parameters, parameters_from_args, parse_args
    from frtm_vos_amd.model.seg_network import SegNetwork
    assert Parameters(None).refiner_precision == 'fp32'
    made = []

    class Stop(Exception):
        pass

    class FakeExtractor:
        def __init__(self, *a, **k):
            pass

        def to(self, device):
            return self

        def get_out_channels(self):
            return dict(FT, layer1=8)

    def fake_tracker(augmenter, extractor, disc_params, refiner, device, **kw):
        made.append(refiner)
        raise Stop
    monkeypatch.setattr(evaluate, 'ResnetFeatureExtractor', FakeExtractor)
    monkeypatch.setattr(evaluate, 'Tracker', fake_tracker)
    for factory in (None, lambda chans: SegNetwork(1, 64, chans, use_bn=True)):
        for argv, want in (([], 'fp32'), (['--refiner-precision', 'bf16x1'], 'bf16x1')):
            args = parse_args(['--model', 'm.pth', '--dset', 'dv2017val', '--dev', 'cpu'] + argv)
            assert args.refiner_precision == want
            p = parameters_from_args(args, None)
            assert p.refiner_precision == want
            p.refiner_factory = factory
            with pytest.raises(Stop):
                p.get_model()
            assert isinstance(made[-1], SegNetwork) and made[-1].precision == want
    assert Parameters(None, refiner_precision='bf16x1').refiner_precision == 'bf16x1'
    with pytest.raises(SystemExit):
        parse_args(['--model', 'm.pth', '--dset', 'dv2017val', '--refiner-precision', 'bf16'])
    with pytest.raises(SystemExit):
        parse_args(['--model', 'm.pth', '--dset', 'dv2017val', '--refiner-precision', 'bf16x3'])
    with pytest.raises(ValueError):
        Parameters(None, refiner_precision='bf16')
