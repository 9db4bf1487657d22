"""Decoder frames without a GPU: the fixed-point colour formula (tests/_decoder_refs.py) against the fp64 matrices and its anchors, the ABI
of frtm_frames_to_rgb_u8, ops.DecoderFrame, the refusals of the ops wrappers, and the register / scratch / LDS budget of
csrc/frame_formats.hip.

Bounds.  The formula's coefficients are the matrices' rounded to 2^-16, so its value before the floor differs from the real one by at most
(239 + 2 * 128) * 2^-17 < 0.004: the two roundings differ by at most 1, and only where the real value lies that close to a tie.  The
differing share is capped at 5e-4 on the sampled grid; on the full 256^3 grid the numpy statement alone stays at or below 2.9e-4."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _decoder_refs as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'


@pytest.mark.parametrize('name', D.NV12)
def test_formula_against_the_fp64_matrix(name):
    Y, U, V = np.meshgrid(np.arange(256), np.arange(0, 256, 5), np.arange(0, 256, 5), indexing='ij')
    got, want = D.yuv_to_rgb(Y, U, V, name), D.yuv_to_rgb_real(Y, U, V, name)
    diff = np.stack([np.abs(g.astype(np.int64) - w.astype(np.int64)) for g, w in zip(got, want)])
    share = float((diff != 0).mean())
    print('%s: max difference %d, differing share %.2e over %d values' % (name, int(diff.max()), share, diff.size))
    assert int(diff.max()) <= 1
    assert share <= 5e-4


@pytest.mark.parametrize('name', D.NV12)
def test_formula_on_the_full_grid_stays_below_its_share(name):
    worst = total = 0
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing='ij')
    for y in range(256):
        Y = np.full_like(U, y)
        got, want = D.yuv_to_rgb(Y, U, V, name), D.yuv_to_rgb_real(Y, U, V, name)
        diff = np.stack([np.abs(g.astype(np.int64) - w.astype(np.int64)) for g, w in zip(got, want)])
        worst, total = max(worst, int(diff.max())), total + int((diff != 0).sum())
    share = total / (3 * 256.0 ** 3)
    print('%s: full grid, max difference %d, differing share %.2e' % (name, worst, share))
    assert worst <= 1 and share <= 2.9e-4


def test_coefficients_are_the_rounded_matrices():
    for name, (_, y0, *ints) in D.FORMATS.items():
        real = D.real_coefficients(name)
        assert y0 == real[0] and ints == [int(round(65536 * c)) for c in real[1:]], name


def test_anchors_and_clamps():
    one = lambda y, u, v, name: [int(c[0]) for c in D.yuv_to_rgb(np.array([y]), np.array([u]), np.array([v]), name)]
    for name in ('nv12_bt601', 'nv12_bt709'):
        assert one(16, 128, 128, name) == [0, 0, 0] and one(235, 128, 128, name) == [255, 255, 255]
        assert one(0, 128, 128, name) == [0, 0, 0] and one(255, 128, 128, name) == [255, 255, 255]        # below black, above white: clamped
    for name in ('nv12_bt601_full', 'nv12_bt709_full'):
        Y = np.arange(256)
        mid = np.full(256, 128)
        for c in D.yuv_to_rgb(Y, mid, mid, name):
            assert np.array_equal(c, Y)
    for name in D.NV12:
        r, g, b = one(128, 0, 255, name)                # chroma at its ends: red saturates, blue is gone
        assert r == 255 and b == 0 and 0 <= g <= 255
        r, g, b = one(128, 255, 0, name)
        assert r == 0 and b == 255 and 0 <= g <= 255
        assert one(255, 255, 255, name)[0] == 255 and one(255, 255, 255, name)[2] == 255
        assert one(0, 0, 0, name)[0] == 0 and one(0, 0, 0, name)[2] == 0
        assert one(0, 255, 255, name)[1] == 0 and one(255, 0, 0, name)[1] == 255


def test_encoder_round_trip_is_close():
    """The encoder only makes inputs; still, a flat picture must come back within the two quantisations."""
    rgb = np.stack([np.full((6, 10), v, dtype=np.uint8) for v in (200, 90, 30)])
    for name in D.NV12:
        buf, uv_off = D.encode_nv12(rgb, 16, name, coded_h=8, fill=77)
        back = D.nv12_to_rgb(buf, 0, 6, 10, 16, uv_off, name)
        assert uv_off == 128 and int(np.abs(back.astype(int) - rgb.astype(int)).max()) <= 3, name
        assert int((buf == 77).sum()) >= (~D.sample_mask(6, 10, 16, 8)).sum() - 3


def test_abi_declares_exports_and_binds_the_entry_point():
    from frtm_vos_amd import _hip, ops
    hdr = open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read()
    assert re.search(r'\bint\s+frtm_frames_to_rgb_u8\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S))
    ids = dict(re.findall(r'#define\s+FRTM_FRAME_(\w+)\s+(\d+)', hdr))
    assert {k.lower(): int(v) for k, v in ids.items()} == ops.FRAME_FORMATS
    assert ops.FRAME_FORMATS == dict(rgb=0, **{name: D.FORMATS[name][0] for name in D.NV12})
    assert hasattr(_hip.lib(), 'frtm_frames_to_rgb_u8')
    res, args = _hip.SIGNATURES['frtm_frames_to_rgb_u8']
    assert res is _hip.I and len(args) == 9                           # src, bytes, two tables, n, out, H, W, stream
    assert callable(ops.frames_to_rgb_u8) and callable(ops.FramePlan) and callable(ops.DecoderFrame)
    assert 'frame_formats.hip' in __import__('frtm_vos_amd.build', fromlist=['SOURCES']).SOURCES


def _fake_cuda_bytes(n):
    """A uint8 'cuda' tensor that owns no memory: DecoderFrame checks its arguments without touching the GPU."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        return torch.empty(n, dtype=torch.uint8, device='cuda')


def test_decoder_frame_defaults_and_shape():
    from frtm_vos_amd import ops
    assert ops.DecoderFrame.layout(7, 13) == (14, 98, 98 + 14 * 4)
    assert ops.DecoderFrame.layout(1080, 1920, 2048, 2048 * 1088) == (2048, 2048 * 1088, 2048 * 1088 + 2048 * 540)
    f = ops.DecoderFrame(_fake_cuda_bytes(200), 7, 13)
    assert (f.pitch, f.uv_offset, f.nbytes_needed, f.format) == (14, 98, 154, ops.FRAME_FORMATS['nv12_bt709'])
    assert f.shape == (3, 7, 13) and tuple(f.shape[-2:]) == (7, 13) and f.dtype == torch.uint8 and f.device.type == 'cuda'
    g = ops.DecoderFrame(_fake_cuda_bytes(16 * 8 + 16 * 3), 6, 10, pitch=16, uv_offset=16 * 8, matrix='bt601', full_range=True)
    assert (g.pitch, g.uv_offset, g.nbytes_needed, g.format) == (16, 128, 176, ops.FRAME_FORMATS['nv12_bt601_full'])
    assert g.row(32, 'cubic') == [32, 6, 10, ops.RESIZE_MODES['cubic'], 2, 16, 160, 0]
    assert ops.DecoderFrame(_fake_cuda_bytes(176), 6, 10, 16, 128, 'bt601').format == 1
    assert ops.DecoderFrame(_fake_cuda_bytes(176), 6, 10, 16, 128, 'bt709', True).format == 4


def test_decoder_frame_refusals():
    from frtm_vos_amd import ops
    ok = _fake_cuda_bytes(200)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.DecoderFrame(torch.zeros(200, dtype=torch.uint8), 7, 13)
    with pytest.raises(TypeError, match='flat uint8'):
        ops.DecoderFrame(torch.zeros(200), 7, 13)
    with pytest.raises(TypeError, match='flat uint8'):
        ops.DecoderFrame(torch.zeros(10, 20, dtype=torch.uint8), 7, 13)
    with pytest.raises(TypeError, match='flat uint8'):
        ops.DecoderFrame(bytes(200), 7, 13)
    for h, w in ((0, 13), (7, 0), (16385, 13), (7, 16385)):
        with pytest.raises(ValueError, match='picture size'):
            ops.DecoderFrame(ok, h, w)
    with pytest.raises(ValueError, match='pitch 13'):
        ops.DecoderFrame(ok, 7, 13, pitch=13)                         # an odd width's chroma row has 14 bytes
    with pytest.raises(ValueError, match='uv_offset'):
        ops.DecoderFrame(ok, 7, 13, pitch=14, uv_offset=97)
    with pytest.raises(ValueError, match='matrix'):
        ops.DecoderFrame(ok, 7, 13, matrix='bt2020')
    with pytest.raises(ValueError, match='needs 154'):
        ops.DecoderFrame(_fake_cuda_bytes(153), 7, 13)


def test_wrappers_refuse_before_any_launch():
    from frtm_vos_amd import ops
    desc = torch.tensor([[0, 6, 10, 0, 3, 16, 128, 0]], dtype=torch.int64)
    cpu = torch.zeros(176, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.frames_to_rgb_u8(cpu, desc, (6, 10))
    fake = _fake_cuda_bytes(176)
    with pytest.raises(TypeError, match='flat uint8'):
        ops.frames_to_rgb_u8(_fake_cuda_bytes(176).view(11, 16), desc, (6, 10))
    with pytest.raises(TypeError, match='flat uint8'):
        from torch._subclasses.fake_tensor import FakeTensorMode
        with FakeTensorMode():
            floats = torch.empty(176, device='cuda')
        ops.frames_to_rgb_u8(floats, desc, (6, 10))
    for bad in (desc.to(torch.int32), desc[:, :4], desc[0], desc[:0], desc.tolist()):
        with pytest.raises(TypeError, match=r'\(n, 8\)'):
            ops.frames_to_rgb_u8(fake, bad, (6, 10))
        with pytest.raises(TypeError, match=r'\(n, 8\)'):
            ops.FramePlan(bad, 'cuda')
    from frtm_vos_amd.model.tracker import Tracker, _tensor_frames_only
    frame = ops.DecoderFrame(fake, 6, 10, 16, 128)
    with pytest.raises(TypeError, match='tensor frames only'):
        _tensor_frames_only('track_window', [cpu, frame])
    with pytest.raises(TypeError, match='tensor frames only'):
        Tracker.track_window(None, [frame], [None])


@pytest.fixture(scope='module')
def formats_isa():
    assert os.path.exists(HIPCC), 'hipcc is needed (the build needs it as well)'
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'frame_formats.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'frame_formats.hip')], check=True, capture_output=True, cwd=d)
        return open(out).read()


def test_kernel_uses_no_scratch_spills_nothing_and_fits_lds(formats_isa):
    kernel = 'k_frames_to_rgb'
    meta = formats_isa[formats_isa.index('amdhsa.kernels:'):]
    blocks = [b for b in meta.split('\n  - ') if re.search(r'\.name:\s+_Z%d%s[A-Z]' % (len(kernel), kernel), b)]
    assert len(blocks) == 1
    b = blocks[0]
    field = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, b).group(1))
    print('%s: %d VGPRs, %d SGPRs, %d bytes of LDS' % (kernel, field('vgpr_count'), field('sgpr_count'), field('group_segment_fixed_size')))
    assert field('vgpr_spill_count') == 0 and field('sgpr_spill_count') == 0
    assert field('private_segment_fixed_size') == 0
    assert 0 < field('group_segment_fixed_size') <= 64 * 1024
    assert not re.search(r'\.uses_dynamic_stack:\s+true', b)
