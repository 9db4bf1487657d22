"""The bf16x1_act trunk mode without a GPU: the ISA of csrc/conv_bf16act.hip (exactly the expected kernels, no scratch, no spills, no atomics, no fp32
MFMA, registers and LDS those of the parent kernels whose occupancy the unit's header claims, the 16-byte staging of a bf16 input), the format plan
(frtm_backbone_act_plan against the rule restated from frtm_backbone_conv_route's answers), the switches and their plumbing, and the layout helpers
of ops against the index formula of include/frtm_hip.h."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from _bf16act_refs import MODES, Trunk, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
# kernel -> (LDS bytes, most VGPRs): the parent form's LDS image and the register budget of the parent's occupancy (conv_bf16x1.hip: 64x64 at four
# workgroups per CU = 128 registers, 128x64 at two = 256; the 3x3 kernels at two workgroups per CU = 256 and at most 80 KB)
KERNELS = {}
for _if in (0, 1):
    KERNELS['k_conv1x1_act<128,64,64,%d>' % _if] = (2 * (8 * 128 + 8 * 64) * 16, 256)
    KERNELS['k_conv1x1_act<64,64,64,%d>' % _if] = (2 * (8 * 64 + 8 * 64) * 16, 128)
    for _fm in (2, 3):
        KERNELS['k_conv3x3_act<%d,%d>' % (_fm, _if)] = (2 * (18 * 32 * _fm + 2 * 10 * 34) * 16, 256)
        KERNELS['k_conv3x3s2_act<%d,%d>' % (_fm, _if)] = ((18 * 32 * _fm + 2 * 17 * 65) * 16, 256)
NEW_SYMBOLS = ('frtm_conv2d_act', 'frtm_conv_bf16act_launches', 'frtm_backbone_set_bf16_act', 'frtm_backbone_act_plan')
FT = {'layer5': 64, 'layer4': 48, 'layer3': 32, 'layer2': 16}
FRAME = (480, 854)


def kernel_name(demangled):
    s = demangled.replace('(anonymous namespace)::', '')
    s = re.sub(r'^void\s+', '', s)
    return s.split('(')[0].replace(' ', '')


@pytest.fixture(scope='module')
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip('no hipcc')
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'conv_bf16act.s')
        p = subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                            os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'conv_bf16act.hip')], capture_output=True, text=True, cwd=d)
        assert p.returncode == 0, p.stderr[-2000:]
        return open(out).read()


def _demangle(names):
    filt = shutil.which('c++filt') or shutil.which('llvm-cxxfilt') or '/opt/rocm/llvm/bin/llvm-cxxfilt'
    assert os.path.exists(filt) or shutil.which(filt), 'c++filt not found'
    res = subprocess.run([filt], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
    return dict(zip(names, (kernel_name(n) for n in res)))


def _bodies(isa):
    out = {}
    for m in re.finditer(r'^(_Z\S+):[^\n]*$(.*?)^\.Lfunc_end', isa, flags=re.M | re.S):
        out[m.group(1)] = m.group(2)
    names = _demangle(list(out))
    return {names[m]: b for m, b in out.items()}


def _metadata(isa):
    """kernel -> {field: int} from the amdhsa.kernels notes."""
    out = {}
    blocks =re.split(r'^  - \.', isa[isa.index('amdhsa.kernels:'):], flags=re.M)[1:]
    mangled = [re.search(r'^\s*\.name:\s+(\S+)', '.' + b, flags=re.M).group(1) for b in blocks]
    names = _demangle(mangled)
    for mg, b in zip(mangled, blocks):
        out[names[mg]] = {k: int(v) for k, v in re.findall(r'\.(vgpr_count|agpr_count|group_segment_fixed_size|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)', '.' + b)}
    return out


def test_kernels_are_exactly_the_expected_ones(isa):
    mangled = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', isa, flags=re.M)
    assert set(_demangle(mangled).values()) == set(KERNELS) and len(mangled) == len(KERNELS)


def test_no_scratch_no_spills_registers_and_lds_of_the_parent_forms(isa):
    meta = _metadata(isa)
    assert set(meta) == set(KERNELS)
    assert set(re.findall(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', isa)) == {'0'}
    for name, (lds, regs) in KERNELS.items():
        m = meta[name]
        assert m['private_segment_fixed_size'] == 0 and m['vgpr_spill_count'] == 0 and m['sgpr_spill_count'] == 0, (name, m)
        assert m['group_segment_fixed_size'] == lds, (name, m)
        assert m['vgpr_count'] <= regs and m['agpr_count'] <= m['vgpr_count'], (name, m)      # (the unified count: accumulation registers included)


@pytest.mark.parametrize('name', sorted(KERNELS))
def test_k_loop_is_bf16_mfma_only_and_a_bf16_input_is_copied(isa, name):
    body = _bodies(isa)[name]
    assert not re.search(r'v_mfma_f32_\w+_f32\b', body), 'an fp32 MFMA'
    assert not re.search(r'global_atomic|buffer_atomic|flat_atomic|ds_\w*(?:add|cmpst|wrxchg)', body), 'an atomic'
    loops = []
    for m in re.finditer(r'^(\.LBB\d+_\d+):', body, flags=re.M):
        lab = m.group(1)
        for j in re.finditer(r's_(?:cbranch_\w+|branch)\s+' + re.escape(lab) + r'\b', body[m.end():]):
            loops.append(body[m.end():m.end() + j.start()])
    assert loops, 'no loop found'
    loop = max(loops, key=lambda b: b.count('v_mfma'))
    args = [int(v) for v in re.findall(r'\d+', name.split('<')[1])]
    if name.startswith('k_conv1x1'):
        want = 2 * 4 * (args[0] // 64)                   # two chunks per trip, four k-steps each, BM / 64 fragments per wave
    else:
        want = 9 * 2 * args[0]                           # nine taps, FM x 2 fragments
    assert loop.count('v_mfma_f32_32x32x16_bf16') == want, (name, loop.count('v_mfma_f32_32x32x16_bf16'))
    assert 's_barrier' in loop and ('ds_read_b128' in loop or 'ds_load_b128' in loop)
    if args[-1]:                                         # bf16 input: 16-byte loads, 16-byte LDS writes, no conversion on the way
        assert 'buffer_load_dwordx4' in loop and 'v_cvt_pk_bf16_f32' not in loop and not re.search(r'buffer_load_dword\s', loop), name
    else:                                                # fp32 input: the parent's staging
        assert loop.count('v_cvt_pk_bf16_f32') >= 8 and re.search(r'buffer_load_dword\s', loop), name


def test_abi_declares_exports_and_binds_the_new_symbols():
    from frtm_vos_amd import _hip, build
    hdr = open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read()
    L = lib()
    for name in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % name, hdr) and name in _hip.SIGNATURES and hasattr(L, name), name
    assert re.search(r'#define\s+FRTM_ACT_FP32\s+0\b', hdr) and re.search(r'#define\s+FRTM_ACT_BF16\s+1\b', hdr)
    assert L.frtm_conv_bf16act_launches() >= 0               # callable without a device
    assert 'conv_bf16act.hip' in build.SOURCES
    assert [k for k, _ in _hip.ConvDesc._fields_] == ['B', 'Cin', 'Hin', 'Win', 'Cout', 'ksize', 'stride', 'pad', 'relu', 'out_transposed', 'splitk',
                                                      'tile', 'w_layout', 'ws_elems', 'w_pitch']      # the descriptor has no new field


# ------------------------------------------------------------------------------------------------------------------------------------------
# The plan
# ------------------------------------------------------------------------------------------------------------------------------------------
def _check_plan(h, B, H, W, on):
    plan = h.plan(B, H, W)
    want, routed, sizes = h.expected_plan(B, H, W, on)
    assert plan == want, [(i, p, w) for i, (p, w) in enumerate(zip(plan, want)) if p != w][:5]
    assert all(v in (0, 1) for f in plan for v in f)
    assert plan[0] == (0, 0, 0)                                          # the stem
    for i, f in enumerate(plan):
        if not routed[i]:
            assert f == (0, 0, 0), (i, f)                                # no fp32-routed conv has a bf16 operand
    for prod, ch, readers, ends in h.tensors(B, H, W):
        for r, how in readers:
            assert plan[prod][2] == plan[r][0 if how == 'in' else 1], (prod, r, how)      # producer and reader agree
        if ends:
            assert plan[prod][2] == 0, prod                              # every stage output is fp32
    return plan, routed, sizes


@pytest.mark.parametrize('arch', (101, 18))
@pytest.mark.parametrize('B', (8, 1))
def test_plan_follows_the_rule_at_the_workload_size(arch, B):
    with Trunk(arch) as h:
        h.mode('bf16x1_act')
        plan, routed, sizes = _check_plan(h, B, FRAME[0], FRAME[1], True)
        shapes = h.shapes()
        assert any(f != (0, 0, 0) for f in plan)
        if B == 8:
            # per stage at least one block output and one block-internal tensor are bf16 in layers 2 to 4 of both trunks
            for s, stage in enumerate(h.blocks(*FRAME)):
                if s == 0 and arch == 101:
                    continue                                             # layer1's 64 -> 256 convs are in no rule: its block outputs stay fp32
                assert any(plan[bl['convs'][0][0]][2] for bl in stage), s
                assert any(plan[bl['convs'][-1][0]][2] for bl in stage[:-1]), s
        if B == 1 and arch == 101:
            # the table leaves the 256-channel 3x3 convs at 30x54, the 512-channel ones at 15x27 and their stride-2 openers fp32 at one frame:
            # whatever they read or write is fp32
            left = [i for i, (co, ci, k, s, p) in enumerate(shapes) if k == 3 and ci == co and ci in (256, 512)]
            assert len(left) == 23 + 3 and not any(routed[i] for i in left)
            for i in left:
                assert plan[i] == (0, 0, 0), (i, plan[i])
            for stage in h.blocks(*FRAME)[2:]:
                for bl in stage:
                    c1, c2, c3 = (i for i, _ in bl['convs'])
                    assert plan[c1][2] == 0 and plan[c3][0] == 0, bl         # t1 and t2 around the fp32 3x3 conv


@pytest.mark.parametrize('arch', (50, 18))
def test_plan_under_min_cols_marks_nearly_every_block_tensor(arch):
    with Trunk(arch, env={'FRTM_BF16X1_MIN_COLS': '0'}) as h:
        h.mode('bf16x1_act')
        plan, routed, sizes = _check_plan(h, 4, 96, 160, True)
        for s, stage in enumerate(h.blocks(96, 160)):
            assert any(plan[bl['convs'][0][0]][2] for bl in stage), s                  # a block-internal tensor
            assert any(plan[bl['convs'][-1][0]][2] for bl in stage[:-1]), s            # a block output


@pytest.mark.parametrize('arch', (101, 18))
def test_plan_is_all_zero_with_the_flag_off_or_not_in_effect(arch):
    L = lib()
    with Trunk(arch, env={'FRTM_BF16X1_MIN_COLS': '0'}) as h:
        n = L.frtm_backbone_num_convs(h.bb)
        for mode in ('fp32', 'bf16x3', 'bf16x1', 'bf16x1_3x3'):
            h.mode(mode)
            for B in (1, 8):
                assert h.plan(B, *FRAME) == [(0, 0, 0)] * n, mode
        # the flag is stored but means nothing without the bf16x1 pieces AND the 3x3 flag
        for pieces, flag in ((0, 0), (3, 1), (1, 0), (0, 1)):
            assert L.frtm_backbone_set_bf16_pieces(h.bb, pieces) == 0 and L.frtm_backbone_set_bf16x1_3x3(h.bb, flag) == 0
            assert L.frtm_backbone_set_bf16_act(h.bb, 1) == 0
            assert h.plan(8, *FRAME) == [(0, 0, 0)] * n, (pieces, flag)
            _check_plan(h, 8, FRAME[0], FRAME[1], False)
        h.mode('bf16x1_act')
        assert h.plan(8, *FRAME) != [(0, 0, 0)] * n


def test_plan_query_refuses_bad_arguments():
    L = lib()
    with Trunk(18) as h:
        n = L.frtm_backbone_num_convs(h.bb)
        buf = (ctypes.c_int * (3 * n))()
        for args in ((None, 1, 480, 854, buf, n), (h.bb, 0, 480, 854, buf, n), (h.bb, 1, 16, 854, buf, n), (h.bb, 1, 480, 854, None, n),
                     (h.bb, 1, 480, 854, buf, n - 1)):
            assert L.frtm_backbone_act_plan(*args) == -1, args[1:4]
            assert b'frtm_backbone_act_plan' in L.frtm_last_error()


# ------------------------------------------------------------------------------------------------------------------------------------------
# Switches and arguments
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_set_bf16_act_validates_without_a_device():
    L = lib()
    with Trunk(18) as h:
        g0 = L.frtm_backbone_generation(h.bb)
        for bad in (2, -1):
            assert L.frtm_backbone_set_bf16_act(h.bb, bad) == -1, bad
            assert b'frtm_backbone_set_bf16_act' in L.frtm_last_error()
            assert L.frtm_backbone_generation(h.bb) == g0
            assert h.plan(4, 96, 160) == [(0, 0, 0)] * L.frtm_backbone_num_convs(h.bb)          # the state is unchanged
        for on, bumps in ((0, 0), (1, 1), (1, 1), (0, 2), (0, 2), (1, 3)):                      # the generation moves when the value changes
            assert L.frtm_backbone_set_bf16_act(h.bb, on) == 0
            assert L.frtm_backbone_generation(h.bb) == g0 + bumps, (on, bumps)
        assert L.frtm_backbone_set_bf16_act(h.bb, 2) == -1 and L.frtm_backbone_generation(h.bb) == g0 + 3
        # stored whatever the other switches are: they keep their own values and bumps, and the flag survives them
        assert L.frtm_backbone_set_bf16_pieces(h.bb, 1) == 0 and L.frtm_backbone_set_bf16x1_3x3(h.bb, 1) == 0
        assert L.frtm_backbone_generation(h.bb) == g0 + 5
        assert L.frtm_backbone_set_bf16_act(h.bb, 1) == 0 and L.frtm_backbone_generation(h.bb) == g0 + 5      # still on
        assert L.frtm_backbone_set_bf16_act(None, 1) == -1


def test_extractor_precision_property_round_trips_without_a_device():
    from frtm_vos_amd.model.feature_extractor import ResnetFeatureExtractor
    ext = ResnetFeatureExtractor('resnet18', seed=0)
    for mode in list(MODES) + ['bf16x1_act']:
        ext.precision = mode
        assert ext.precision == mode
    for bad in ('bf16', 'bf16_act', 'bf16x1_ACT', 'bf16x3_act', None):
        with pytest.raises(ValueError):
            ext.precision = bad
        assert ext.precision == 'bf16x1_act'
    assert ResnetFeatureExtractor('resnet18', seed=0, precision='bf16x1_act').precision == 'bf16x1_act'
    with pytest.raises(ValueError):
        ResnetFeatureExtractor('resnet18', precision='bf16x1_ac')


def test_extractor_moves_the_storage_switch_only_when_it_changes(monkeypatch):
    from frtm_vos_amd.model import feature_extractor as FE
    calls = []
    monkeypatch.setattr(FE.H, 'call_nostream', lambda name, handle, *a: calls.append((name,) + a))
    ext = FE.ResnetFeatureExtractor('resnet18', seed=0)
    P, F3, A = 'frtm_backbone_set_bf16_pieces', 'frtm_backbone_set_bf16x1_3x3', 'frtm_backbone_set_bf16_act'
    for mode, want in (('bf16x1_3x3', [(P, 1), (F3, 1)]), ('bf16x1_act', [(P, 1), (F3, 1), (A, 1)]), ('bf16x1_act', [(P, 1), (F3, 1)]),
                       ('bf16x1_3x3', [(P, 1), (F3, 1), (A, 0)]), ('bf16x1_act', [(P, 1), (F3, 1), (A, 1)]), ('fp32', [(P, 0), (F3, 0), (A, 0)]),
                       ('bf16x3', [(P, 3), (F3, 0)])):
        del calls[:]
        ext._apply_precision(mode)
        assert calls == want, (mode, calls)


def test_parameters_and_evaluate_command_line_reach_the_extractor(monkeypatch):
    from frtm_vos_amd import evaluate
    from frtm_vos_amd.evaluate import Parameters, parameters_from_args, parse_args
    from frtm_vos_amd.model import feature_extractor as FE
    seen = []

    class Stop(Exception):
        pass

    def fake_init(self, name, weights=None, seed=0, precision='fp32'):
        seen.append((name, precision))
        raise Stop
    monkeypatch.setattr(FE.ResnetFeatureExtractor, '__init__', fake_init)
    monkeypatch.setattr(evaluate, 'ResnetFeatureExtractor', FE.ResnetFeatureExtractor)
    args = parse_args(['--model', 'm.pth', '--dset', 'dv2017val', '--trunk-precision', 'bf16x1_act'])
    assert args.trunk_precision == 'bf16x1_act'
    p = parameters_from_args(args, None)
    assert p.trunk_precision == 'bf16x1_act'
    with pytest.raises(Stop):
        p.get_model()
    assert seen[-1][1] == 'bf16x1_act'
    p = Parameters(None, fast=True, feature_extractor='resnet18', trunk_precision='bf16x1_act')
    with pytest.raises(Stop):
        p.get_model()
    assert seen[-1] == ('resnet18', 'bf16x1_act')
    for bad in ('bf16', 'bf16_act', 'bf16x1_ac'):
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
    args = train.parse_args(['name', '--dev', 'cpu', '--trunk-precision', 'bf16x1_act'])
    assert args.trunk_precision == 'bf16x1_act'
    p = train.ModelParameters(args.name, device=args.dev, trunk_precision=args.trunk_precision)
    assert p.trunk_precision == 'bf16x1_act'
    with pytest.raises(Stop):
        p.get_model()
    assert made[-1] == 'bf16x1_act'
    with pytest.raises(SystemExit):
        train.parse_args(['name', '--trunk-precision', 'bf16_act'])
    with pytest.raises(ValueError):
        train.ModelParameters('n', trunk_precision='bf16_act')
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
        train.main(['name', '--dev', 'cpu', '--trunk-precision', 'bf16x1_act'])
    assert seen['trunk_precision'] == 'bf16x1_act'


# ------------------------------------------------------------------------------------------------------------------------------------------
# The layout helpers
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_layout_helpers_match_the_index_formula():
    import torch
    from frtm_vos_amd import ops
    B, C, H, W = 2, 16, 3, 5
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(3))
    buf = ops.act_to_bf16(x)
    assert buf.dtype == torch.bfloat16 and buf.shape == (B * C * H * W,)
    want = x.to(torch.bfloat16)                            # nearest even
    for img in range(B):
        for c in range(C):
            for p in range(H * W):
                at = ((img * (C // 8) + c // 8) * H * W + p) * 8 + c % 8
                assert buf[at] == want[img, c, p // W, p % W], (img, c, p)
    back = ops.act_from_bf16(buf, (B, C, H, W))
    assert back.dtype == torch.float32 and back.shape == (B, C, H, W) and torch.equal(back, want.float())
    special = torch.zeros(1, 8, 1, 2)
    special[0, 0, 0, 0], special[0, 1, 0, 0], special[0, 2, 0, 0] = float('nan'), float('inf'), -float('inf')
    got = ops.act_from_bf16(ops.act_to_bf16(special), (1, 8, 1, 2))
    assert torch.isnan(got[0, 0, 0, 0]) and got[0, 1, 0, 0] == float('inf') and got[0, 2, 0, 0] == -float('inf')
    with pytest.raises(ValueError):
        ops.act_to_bf16(torch.zeros(1, 12, 2, 2))
    with pytest.raises(ValueError):
        ops.act_from_bf16(buf, (B, C, H, W + 1))
