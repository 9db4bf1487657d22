"""CPU side of the per-kernel checks of csrc/refiner_ops.hip and csrc/refiner_train.hip.

(a) The float64 references of tests/_refiner_refs.py, composed the way SegNetwork.forward_torch composes its modules, reproduce the
    .double() TSE, CAB and head modules to float64 rounding (<= 1e-12 * max|ref|), and the backward references equal autograd through
    those modules.  The GPU tests (tests/test_refiner_kernels_gpu.py) hold every kernel to these references.
(b) COVERED names, for every __global__ of the two files, the tests that call it directly.  The entries of this module's GPU
    counterpart and of tests/test_refiner_train_gpu.py hold the kernel to a float64 definition; k_project_tail, k_bicubic_resize and
    k_project_tail_bicubic map to their existing direct tests, which compare with fp32 PyTorch (and the unfused HIP kernels) under
    scalar gates of 1e-5 to 2e-6.  A kernel added without an entry fails test_every_kernel_is_covered.
(c) One definition per launch and rule: the two model files name no C entry point, frtm_project_tail_fits is the literal fit rule over
    every size of either axis, and each ops.py wrapper of a glue kernel refuses, on CPU tensors, what the C side cannot see.
"""
import ast
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _refiner_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'frtm-vos_amd', 'csrc')
NEW = 'tests/test_refiner_kernels_gpu.py::'
TRAIN = 'tests/test_refiner_train_gpu.py::'
HEAD = 'tests/test_upsampler_head_gpu.py::'

COVERED = {
    # refiner_ops.hip
    'k_bilinear_resize': [NEW + 'test_bilinear_resize'],
    'k_tse_inject': [NEW + 'test_tse_inject'],
    'k_cab_combine': [NEW + 'test_cab_combine'],
    'k_cab_gate': [NEW + 'test_cab_gate'],
    'k_pyrup2x': [NEW + 'test_pyrup2x', NEW + 'test_pyrup2x_grid_stride_second_trip'],
    'k_plane_mean': [NEW + 'test_plane_mean'],
    'k_tap_mix': [NEW + 'test_tap_mix', NEW + 'test_tap_mix_misaligned'],
    'k_project_tail': ['tests/test_hip_parity.py::test_project_tail_fused'],
    'k_bicubic_resize': [HEAD + 'test_bicubic_resize_vs_interpolate'],
    'k_project_tail_bicubic': [HEAD + 'test_project_tail_bicubic_fused_vs_unfused'],
    # refiner_train.hip
    'k_conv_wgrad': [TRAIN + 'test_conv_wgrad'],
    'k_conv_wgrad_reduce': [TRAIN + 'test_conv_wgrad'],
    'k_bn_stats_part': [TRAIN + 'test_batchnorm_relu'],
    'k_bn_stats_final': [TRAIN + 'test_batchnorm_relu'],
    'k_bn_apply_relu': [TRAIN + 'test_batchnorm_relu'],
    'k_bn_bwd_part': [TRAIN + 'test_batchnorm_relu'],
    'k_bn_bwd_apply': [TRAIN + 'test_batchnorm_relu'],
    'k_pyrup2x_bwd_axis': [TRAIN + 'test_pyrup2x_backward'],
    'k_bilinear_bwd_axis': [TRAIN + 'test_bilinear_backward'],
    'k_relu_bwd': [NEW + 'test_relu_backward'],
    'k_cab_bwd_reduce': [NEW + 'test_cab_backward_reduce'],
    'k_cab_gate_bwd': [NEW + 'test_cab_gate_backward', NEW + 'test_cab_gate_backward_frozen_weights'],
    'k_cab_bwd_shallow': [NEW + 'test_cab_backward_shallow'],
    'k_add_plane': [NEW + 'test_add_plane'],
    'k_shift9': [NEW + 'test_shift9'],
}


GLOBAL_DECL = r'__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?void\s+(\w+)\s*\('


def _kernels(name):
    return set(re.findall(GLOBAL_DECL, open(os.path.join(CSRC, name)).read()))


def test_every_kernel_is_covered():
    found = _kernels('refiner_ops.hip') | _kernels('refiner_train.hip')
    assert len(found) >= 25, sorted(found)                       # the pattern still reads the files
    assert found == set(COVERED), 'without a test: %s; no such kernel: %s' % (sorted(found - set(COVERED)), sorted(set(COVERED) - found))
    for k, ids in COVERED.items():
        assert ids, k
        for tid in ids:
            path, name = tid.split('::')
            tree = ast.parse(open(os.path.join(ROOT, path)).read())
            assert name in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, tid


def test_kernel_pattern_reads_templates_and_bounds():
    src = 'template <int V>\n__global__ __launch_bounds__(256, 4) void k_a(int x) {}\n__global__ void k_b(\n'
    assert re.findall(GLOBAL_DECL, src) == ['k_a', 'k_b']


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) the references against the float64 modules
# ---------------------------------------------------------------------------------------------------------------------------------
def _close(a, b, what):
    e, m = float((a - b).abs().max()), float(b.abs().max())
    assert a.shape == b.shape and e <= 1e-12 * m, '%s: err %.3e, max|ref| %.3e' % (what, e, m)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def test_pyr_taps_are_the_module_taps():
    from frtm_vos_amd.model.seg_network import PyrUpBicubic2d
    assert torch.equal(torch.tensor(R.PYR_TAPS, dtype=torch.float64), PyrUpBicubic2d(1).taps.double())
    assert R.PYR_TAPS[0] == [-27 / 256, 225 / 256, 67 / 256, -9 / 256] and R.PYR_TAPS[1] == R.PYR_TAPS[0][::-1]


@pytest.mark.parametrize('h,w', [(1, 1), (1, 5), (2, 3), (4, 1), (7, 9), (13, 17)])
def test_pyrup2x_reference(h, w):
    from frtm_vos_amd.model.seg_network import PyrUpBicubic2d
    x = _rand(_gen(h * 31 + w), 2, 3, h, w)
    _close(R.pyrup2x(x.reshape(6, h, w)).reshape(2, 3, 2 * h, 2 * w), PyrUpBicubic2d(3).double()(x), 'pyrup2x')


@pytest.mark.parametrize('group,frames,half', [(1, 1, False), (2, 2, True), (3, 1, True)])
def test_tse_reference(group, frames, half):
    from frtm_vos_amd.model.seg_network import TSE
    g = _gen(11 + group)
    torch.manual_seed(3)
    oc, Hh, Ww = 6, 9, 13
    tse = TSE(10, 1, oc).double()
    n = frames * group
    ft = _rand(g, frames, 10, Hh, Ww)
    scores = _rand(g, n, 1, (Hh + 1) // 2, (Ww + 1) // 2) if half else _rand(g, n, 1, Hh, Ww)
    with torch.no_grad():
        h = tse.reduce(ft)
        # forward_torch: red.repeat_interleave(group), interpolate(scores), transform[0] on the concatenation, relu
        s = scores if not half else F.interpolate(scores, (Hh, Ww), mode='bilinear', align_corners=False)
        want = tse.transform[1](tse.transform[0](torch.cat((h.repeat_interleave(group, 0), s), 1)))
        w0 = tse.transform[0].weight
        base = F.conv2d(h, w0[:, :oc], padding=1)
        got = R.tse_inject(base, tse.transform[0].bias, w0[:, oc].reshape(-1, 9), scores[:, 0], group)
    _close(got, want, 'tse_inject')
    with torch.no_grad():                                      # ... and the whole module from there
        _close(tse.transform[2:](got), tse(h.repeat_interleave(group, 0), s), 'TSE')


def _cab_forward(cab, deeper, shallower, group):
    """CAB.forward from the references; deeper (frames,oc) pooled vector when deepest, else (n,oc,hd,wd)."""
    n, oc, Hh, Ww = shallower.shape
    c = cab.convreluconv
    sp = R.plane_mean(shallower.reshape(n * oc, -1)).view(n, oc)
    if cab.deepest:
        dp, dmap = deeper, deeper[:, :, None, None]
    else:
        dp, dmap = R.plane_mean(deeper.reshape(n * oc, -1)).view(n, oc), deeper
    gate = R.cab_gate(sp, dp, group, c[0].weight.flatten(1).t(), c[0].bias, c[2].weight.flatten(1).t(), c[2].bias)
    return R.cab_combine(shallower, gate, dmap, group), sp, dp, gate


@pytest.mark.parametrize('deepest,group,hd,wd', [(True, 1, 1, 1), (True, 3, 1, 1), (False, 0, 5, 7), (False, 0, 9, 13), (False, 0, 4, 20)])
def test_cab_reference_forward_and_backward(deepest, group, hd, wd):
    from frtm_vos_amd.model.seg_network import CAB
    g = _gen(5 + hd)
    torch.manual_seed(4)
    oc, Hh, Ww = 8, 9, 13
    frames = 2
    n = frames * max(group, 1)
    cab = CAB(oc, deepest).double()
    c = cab.convreluconv
    shallower = _rand(g, n, oc, Hh, Ww).requires_grad_()
    dout = _rand(g, n, oc, Hh, Ww)
    if deepest:
        pool = _rand(g, frames, oc).requires_grad_()
        deeper = pool.repeat_interleave(group, 0)[:, :, None, None]       # forward_torch: pool.repeat_interleave(group, 0)
    else:
        deeper = pool = _rand(g, n, oc, hd, wd).requires_grad_()
    want = cab(deeper, shallower)
    with torch.no_grad():
        got, sp, dp, gate = _cab_forward(cab, pool.detach(), shallower.detach(), group)
    _close(got, want.detach(), 'CAB')
    params = [c[0].weight, c[0].bias, c[2].weight, c[2].bias]
    auto = torch.autograd.grad(want, params + [shallower, pool], dout)
    # the backward as model/refiner_train.py composes it
    a, b = R.cab_backward_reduce(dout.reshape(n * oc, -1), shallower.detach().reshape(n * oc, -1))
    a, b = a.view(n, oc), b.view(n, oc)
    dpn = dp.repeat_interleave(group, 0) if deepest else dp
    dW1, db1, dW2, db2, dsp, ddp = R.cab_gate_backward(sp, dpn, gate, a, b if deepest else None, c[0].weight.detach().flatten(1),
                                                       c[0].bias.detach(), c[2].weight.detach().flatten(1))
    ds = R.cab_backward_shallow(dout.reshape(n * oc, -1), gate.reshape(-1), dsp.reshape(-1)).view(n, oc, Hh, Ww)
    if deepest:
        dpool = ddp.view(frames, group, oc).sum(1)                           # the objects of a frame share the pooled vector
    else:
        x = pool.detach().clone().requires_grad_()
        up = x if (hd, wd) == (Hh, Ww) else F.interpolate(x, (Hh, Ww), mode='bilinear', align_corners=False)
        dx = torch.autograd.grad(up, x, dout)[0]
        dpool = R.add_plane(dx.reshape(n * oc, -1), ddp.reshape(-1), 1.0 / (hd * wd)).view(n, oc, hd, wd)
    for got_, want_, what in zip((dW1.view_as(auto[0]), db1, dW2.view_as(auto[2]), db2, ds, dpool), auto, ('dW1', 'db1', 'dW2', 'db2', 'ds', 'dd')):
        _close(got_, want_, what)


def test_cab_reference_same_size_deeper():
    from frtm_vos_amd.model.seg_network import CAB
    g = _gen(8)
    torch.manual_seed(4)
    cab = CAB(4, False).double()
    s, d = _rand(g, 2, 4, 6, 5), _rand(g, 2, 4, 6, 5)
    with torch.no_grad():
        _close(_cab_forward(cab, d, s, 0)[0], cab(d, s), 'CAB same size')


@pytest.mark.parametrize('size', [(36, 52), (33, 50), (40, 61)])
def test_head_reference(size):
    """BackwardCompatibleUpsampler from pyrup2x / bilinear_resize, directly and on conv2's nine tap maps (tap_mix), and the tail's
    backward: conv2's input gradient from shift9."""
    from frtm_vos_amd.model.seg_network import BackwardCompatibleUpsampler
    g = _gen(size[0])
    torch.manual_seed(6)
    n, C, h, w = 2, 8, 9, 13
    head = BackwardCompatibleUpsampler(C).double()
    x = _rand(g, n, C, h, w)
    Ho, Wo = size
    with torch.no_grad():
        want = head(x, size)
        u1 = R.pyrup2x(x.reshape(n * C, h, w)).view(n, C, 2 * h, 2 * w)
        y = F.relu(F.conv2d(u1, head.conv1.weight, head.conv1.bias, padding=1))
        c2 = y.shape[1]
        u2 = R.pyrup2x(y.reshape(n * c2, 2 * h, 2 * w))
        z = R.bilinear_resize(u2, Ho, Wo).view(n, c2, Ho, Wo)
        _close(F.conv2d(z, head.conv2.weight, head.conv2.bias, padding=1), want, 'head')
        ym = R.tap_mix(y.reshape(n, c2, -1), head.conv2.weight.reshape(c2, 9)).reshape(n * 9, 2 * h, 2 * w)
        zm = R.bilinear_resize(R.pyrup2x(ym), Ho, Wo).view(n, 9, Ho, Wo)
        _close(F.conv2d(zm, torch.eye(9, dtype=torch.float64).view(1, 9, 3, 3), head.conv2.bias, padding=1), want, 'head on tap maps')
    dl = _rand(g, n, 1, Ho, Wo)
    zz = z.clone().requires_grad_()
    auto = torch.autograd.grad(F.conv2d(zz, head.conv2.weight.detach(), padding=1), zz, dl)[0]
    S = R.shift9(dl[:, 0])
    _close(torch.einsum('ct,nthw->nchw', head.conv2.weight.detach().reshape(c2, 9), S), auto, 'conv2 input gradient from shift9')


def test_relu_backward_reference():
    y = torch.tensor([-1.0, -0.0, 0.0, 1e-300, 2.0], dtype=torch.float64)
    dy = torch.tensor([3.0, 4.0, 5.0, 6.0, -7.0], dtype=torch.float64)
    assert torch.equal(R.relu_backward(dy, y), torch.tensor([0.0, 0.0, 0.0, 6.0, -7.0], dtype=torch.float64))
    x = torch.tensor([-1.0, 0.5, 2.0], dtype=torch.float64, requires_grad=True)
    out = F.leaky_relu(x, 0.0)                                      # lib/utils.py: relu() is LeakyReLU(0)
    up = torch.tensor([3.0, 4.0, 5.0], dtype=torch.float64)
    assert torch.equal(R.relu_backward(up, out.detach()), torch.autograd.grad(out, x, up)[0])


def test_add_plane_reference_is_the_mean_backward():
    g = _gen(2)
    x0, v = _rand(g, 3, 35), _rand(g, 3)
    x = x0.clone().requires_grad_()
    auto = torch.autograd.grad(x.mean(1), x, v)[0]
    _close(R.add_plane(x0, v, 1.0 / 35), x0 + auto, 'add_plane')


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) one definition per launch and per rule: the model files launch through ops.py, the fit rule is the library's, and the wrappers refuse
#     what the C side cannot see
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['seg_network.py', 'refiner_train.py'])
def test_model_files_launch_through_ops(name):
    """No C entry point is named in a string literal of the two model files: every glue launch goes through its ops.py wrapper."""
    src = open(os.path.join(ROOT, 'frtm-vos_amd', 'model', name)).read()
    assert len(src) > 5000
    assert re.findall(r'''['"]frtm_\w*''', src) == []


def _fit_literal(bicubic, h, w, Ho, Wo):
    if bicubic:
        return int(17 * (h / Ho)) + 6 <= 16 and int(65 * (w / Wo)) + 6 <= 40
    return int(18 * (2.0 * h / Ho)) + 3 <= 22 and int(66 * (2.0 * w / Wo)) + 3 <= 76


@pytest.mark.parametrize('axis', ['rows', 'columns'])
@pytest.mark.parametrize('bicubic', [0, 1])
def test_project_tail_fits_is_the_literal_rule(bicubic, axis):
    """frtm_project_tail_fits over every map size 2 ... 800 (even) and output size 1 ... 2400 of one axis, the other axis at a size that fits
    (rows and columns are independent factors of the rule), and with the other axis at one that does not."""
    from frtm_vos_amd import _hip as H
    fits = H.lib().frtm_project_tail_fits
    assert _fit_literal(bicubic, 2, 2, 4, 4) and not _fit_literal(bicubic, 2, 2, 1, 1)
    bad = []
    for a in range(2, 801, 2):
        for o in range(1, 2401):
            args = (a, 2, o, 4) if axis == 'rows' else (2, a, 4, o)
            if bool(fits(bicubic, *args)) != _fit_literal(bicubic, *args):
                bad.append(args)
        args = (a, 2, 2 * a, 1) if axis == 'rows' else (2, a, 1, 2 * a)             # this axis fits, the other does not
        assert _fit_literal(bicubic, a, a, 2 * a, 2 * a) and not fits(bicubic, *args)
    assert bad == [], bad[:10]
    if not bicubic:      # the spelling the two model files used before they asked the library (hh = h / 2, the map before conv1's 2x step)
        k, lim = (18, 22) if axis == 'rows' else (66, 76)
        assert all((int(k * 4.0 * (a // 2) / o) + 3 <= lim) == (int(k * (2.0 * a / o)) + 3 <= lim) for a in range(2, 801, 2) for o in range(1, 2401))
    assert not fits(bicubic, 0, 2, 4, 4) and not fits(bicubic, 2, 2, 0, 4)


def test_project_tail_fits_wrappers():
    from frtm_vos_amd import ops
    from frtm_vos_amd.model.seg_network import bicubic_tail_fits
    for h, w, Ho, Wo in ((240, 428, 480, 854), (240, 428, 240, 427), (56, 76, 90, 150), (28, 38, 30, 45), (240, 428, 481, 854)):
        assert ops.project_tail_fits(h, w, (Ho, Wo)) == _fit_literal(0, h, w, Ho, Wo)
        assert ops.project_tail_fits(h, w, (1, 3, Ho, Wo), bicubic=True) == _fit_literal(1, h, w, Ho, Wo) == bicubic_tail_fits(h, w, Ho, Wo)


def test_wino_launch_rule():
    from frtm_vos_amd import ops
    assert ops.WINO_MIN_BLOCKS == int(re.search(r'#define FRTM_WINO_MIN_BLOCKS (\d+)', open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read()).group(1))
    assert ops.wino_launch(4, 120, 214, 64) and not ops.wino_launch(4, 30, 54, 64)
    assert ops.wino_launch(2, 60, 107, 64) is False and ops.wino_launch(3, 60, 107, 64) is True      # 448 and 672 blocks
    assert ops.wino_launch(8, 57, 57, 33) and not ops.wino_launch(8, 56, 56, 32)                      # 1024 (rounded up) and 392


def _t(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype)


# n = 6 samples in groups of 3, C = 8 channels, maps 5 x 7 -> 9 x 13, image 18 x 26; every call differs from a valid one in one argument
_N, _G, _C = 6, 3, 8
_GATE_W = lambda: (_t(2 * _C, _C), _t(_C), _t(_C, _C), _t(_C))
_GB = lambda **k: dict(dict(sp=_t(_N, _C), dp=_t(_N, _C), gate=_t(_N, _C), a=_t(_N, _C), badd=None, w1=_t(_C, 2 * _C, 1, 1), b1=_t(_C), w2=_t(_C, _C, 1, 1)), **k)
REFUSALS = [
    ('plane_mean', lambda o: o.plane_mean(_t(_N, _C, 9)), ValueError),
    ('plane_mean', lambda o: o.plane_mean(_t(_N, _C, 9, 13, dtype=torch.float64)), TypeError),
    ('pyrup2x', lambda o: o.pyrup2x(_t(_C, 5, 7)), ValueError),
    ('pyrup2x', lambda o: o.pyrup2x(_t(_N, _C, 5, 7, dtype=torch.float16)), TypeError),
    ('bicubic_resize', lambda o: o.bicubic_resize(_t(_N * _C, 5, 7), (9, 13)), ValueError),
    ('bicubic_resize', lambda o: o.bicubic_resize(_t(_N, _C, 5, 7), (0, 13)), ValueError),
    ('bicubic_resize', lambda o: o.bicubic_resize(_t(_N, _C, 5, 7).int(), (9, 13)), TypeError),
    ('tse_inject', lambda o: o.tse_inject(_t(2, _C, 9, 13), _t(_C), _t(_C, 9), _t(_N, 1, 5, 7), 2), ValueError),          # 2 frames x 2 != 6
    ('tse_inject', lambda o: o.tse_inject(_t(2, _C, 9, 13), _t(_C), _t(_C, 9), _t(_N, 1, 5, 7), 4), ValueError),          # 6 % 4
    ('tse_inject', lambda o: o.tse_inject(_t(2, _C, 9, 13), _t(_C), _t(_C, 9), _t(_N, 2, 5, 7), _G), ValueError),         # two score channels
    ('tse_inject', lambda o: o.tse_inject(_t(2, _C, 9, 13), _t(_C), _t(_C, 9), _t(_N, 5, 7), _G), ValueError),            # rank
    ('tse_inject', lambda o: o.tse_inject(_t(2, _C, 9, 13), _t(_C + 1), _t(_C, 9), _t(_N, 1, 5, 7), _G), ValueError),     # bias channels
    ('tse_inject', lambda o: o.tse_inject(_t(2, _C, 9, 13), _t(_C), _t(_C, 3), _t(_N, 1, 5, 7), _G), ValueError),         # taps
    ('tse_inject', lambda o: o.tse_inject(_t(2, _C, 9, 13), _t(_C), _t(_C, 9), _t(_N, 1, 5, 7), 0), ValueError),
    ('tse_inject', lambda o: o.tse_inject(_t(2, _C, 9, 13), _t(_C), _t(_C, 9).double(), _t(_N, 1, 5, 7), _G), TypeError),
    ('cab_gate', lambda o: o.cab_gate(_t(_N, _C), _t(_N, _C + 4), *_GATE_W()), ValueError),                               # channels differ
    ('cab_gate', lambda o: o.cab_gate(_t(_N, _C), _t(3, _C), *_GATE_W(), dp_group=_G), ValueError),                       # 3 rows, 6 / 3 = 2
    ('cab_gate', lambda o: o.cab_gate(_t(_N, _C), _t(2, _C), *_GATE_W(), dp_group=0), ValueError),
    ('cab_gate', lambda o: o.cab_gate(_t(_N, _C), _t(_N, _C), *_GATE_W(), dp_group=-1), ValueError),
    ('cab_gate', lambda o: o.cab_gate(_t(_N, _C), _t(_N, _C), _t(_C, 2 * _C), _t(_C), _t(_C, _C), _t(_C)), ValueError),   # w1 not transposed
    ('cab_gate', lambda o: o.cab_gate(_t(_N, _C), _t(_N, _C), _t(2 * _C, _C), _t(_C), _t(_C, _C), _t(_C + 1)), ValueError),
    ('cab_gate', lambda o: o.cab_gate(_t(_N, 6), _t(_N, 6), _t(12, 6), _t(6), _t(6, 6), _t(6)), ValueError),              # oc % 4
    ('cab_gate', lambda o: o.cab_gate(_t(_N, _C, 1, 1), _t(_N, _C), *_GATE_W()), ValueError),
    ('cab_gate', lambda o: o.cab_gate(_t(_N, _C), _t(_N, _C).double(), *_GATE_W()), TypeError),
    ('cab_combine', lambda o: o.cab_combine(_t(_N, _C, 9, 13), _t(_N, _C + 1), _t(_N, _C, 5, 7)), ValueError),
    ('cab_combine', lambda o: o.cab_combine(_t(_N, _C, 9, 13), _t(_N, _C), _t(_N, _C + 1, 5, 7)), ValueError),
    ('cab_combine', lambda o: o.cab_combine(_t(_N, _C, 9, 13), _t(_N, _C), _t(2, _C, 5, 7)), ValueError),                 # 2 deeper maps, group 0
    ('cab_combine', lambda o: o.cab_combine(_t(_N, _C, 9, 13), _t(_N, _C), _t(3, _C), deeper_group=_G), ValueError),      # pooled: 3 rows, 6 / 3 = 2
    ('cab_combine', lambda o: o.cab_combine(_t(_N, _C, 9, 13), _t(_N, _C), _t(2, _C), deeper_group=4), ValueError),
    ('cab_combine', lambda o: o.cab_combine(_t(_N, _C, 9, 13), _t(_N, _C), _t(_N, _C, 5)), ValueError),                   # rank 3
    ('cab_combine', lambda o: o.cab_combine(_t(_N, _C, 9, 13), _t(_N, _C), _t(_N, _C, 5, 7).half()), TypeError),
    ('tap_mix', lambda o: o.tap_mix(_t(_N, _C, 9, 13), _t(1, _C + 1, 3, 3)), ValueError),
    ('tap_mix', lambda o: o.tap_mix(_t(_N, _C, 9 * 13), _t(1, _C, 3, 3)), ValueError),
    ('tap_mix', lambda o: o.tap_mix(_t(_N, _C, 9, 13), _t(1, _C, 3, 3).double()), TypeError),
    ('project_tail', lambda o: o.project_tail(_t(_N, 9, 9, 13), _t(1, _C, 3, 3), _t(1), (18, 26)), ValueError),             # weights of 8 channels, 9 maps
    ('project_tail', lambda o: o.project_tail(_t(_N, _C, 9, 13), _t(1, _C, 3, 3), _t(2), (18, 26)), ValueError),
    ('project_tail', lambda o: o.project_tail(_t(_N, _C, 9, 13), _t(1, _C, 3, 3), None, (18, 0), bicubic=True), ValueError),
    ('project_tail', lambda o: o.project_tail(_t(_N * _C, 9, 13), _t(1, _C, 3, 3), None, (18, 26)), ValueError),
    ('project_tail', lambda o: o.project_tail(_t(_N, _C, 9, 13).double(), _t(1, _C, 3, 3), None, (18, 26)), TypeError),
    ('shift9', lambda o: o.shift9(_t(_N, 2, 18, 26)), ValueError),
    ('shift9', lambda o: o.shift9(_t(_N, 18, 26)), ValueError),
    ('shift9', lambda o: o.shift9(_t(_N, 1, 18, 26).double()), TypeError),
    ('cab_backward_reduce', lambda o: o.cab_backward_reduce(_t(_N, _C, 9, 13), _t(_N, _C, 13, 9)), ValueError),
    ('cab_backward_reduce', lambda o: o.cab_backward_reduce(_t(_N, _C, 9, 13), _t(_N * _C, 9 * 13)), ValueError),
    ('cab_backward_reduce', lambda o: o.cab_backward_reduce(_t(_N, _C, 9, 13), _t(_N, _C, 9, 13).double()), TypeError),
    ('cab_gate_backward', lambda o: o.cab_gate_backward(**_GB(dp=_t(2, _C))), ValueError),
    ('cab_gate_backward', lambda o: o.cab_gate_backward(**_GB(gate=_t(_C, _N))), ValueError),
    ('cab_gate_backward', lambda o: o.cab_gate_backward(**_GB(badd=_t(_N, _C, 1))), ValueError),
    ('cab_gate_backward', lambda o: o.cab_gate_backward(**_GB(w1=_t(_C, _C, 1, 1))), ValueError),
    ('cab_gate_backward', lambda o: o.cab_gate_backward(**_GB(w2=_t(_C, 2 * _C, 1, 1))), ValueError),
    ('cab_gate_backward', lambda o: o.cab_gate_backward(**_GB(b1=_t(2 * _C))), ValueError),
    ('cab_gate_backward', lambda o: o.cab_gate_backward(**_GB(a=_t(_N, _C).double())), TypeError),
    ('cab_backward_shallow', lambda o: o.cab_backward_shallow(_t(_N, _C, 9, 13), _t(_N, _C + 1), _t(_N, _C)), ValueError),
    ('cab_backward_shallow', lambda o: o.cab_backward_shallow(_t(_N, _C, 9, 13), _t(_N, _C), _t(_N * _C)), ValueError),
    ('cab_backward_shallow', lambda o: o.cab_backward_shallow(_t(_N, _C, 9, 13), _t(_N, _C), _t(_N, _C).double()), TypeError),
]


@pytest.mark.parametrize('i', range(len(REFUSALS)), ids=['%s-%d' % (r[0], i) for i, r in enumerate(REFUSALS)])
def test_wrapper_refuses_before_any_device_check(i):
    """CPU tensors and no launch: the shape, group and dtype checks come before anything that needs a device, and the message names the wrapper."""
    from frtm_vos_amd import ops
    name, call, exc = REFUSALS[i]
    with pytest.raises(exc, match='^' + name + ': '):
        call(ops)


def test_every_new_wrapper_has_a_refusal_case():
    assert {r[0] for r in REFUSALS} == {'plane_mean', 'pyrup2x', 'bicubic_resize', 'tse_inject', 'cab_gate', 'cab_combine', 'tap_mix', 'project_tail',
                                        'shift9', 'cab_backward_reduce', 'cab_gate_backward', 'cab_backward_shallow'}
    assert all(any(r[0] == n and r[2] is e for r in REFUSALS) for n in {r[0] for r in REFUSALS} for e in (ValueError, TypeError))
