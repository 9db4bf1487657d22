"""The renderer without a GPU (csrc/frame_render.hip, ops.RenderStyle / render_frames): the ABI, the refusals of the C entry (they
run on the host, before any launch), the numpy statement of tests/_render_refs.py against exact arithmetic, RenderStyle's tables and its
refusals, and the kernel's scratch / spill / LDS budget.  The kernel itself is checked on the GPU (tests/test_frame_render_gpu.py).

Bounds.  mix is claimed to BE round-half-up of s + (c - s) a / 255, so it is held to equality on all 256^3 inputs.  The forward colour
table's coefficients are the matrices' rounded to 2^-16: before the rounding to an integer the fixed-point value differs from the real one
by at most 3 * 255 * 2^-17 < 0.006, so the two roundings differ by at most 1 (the bar the issue sets), wherever the real value lies that
close to a tie."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _decoder_refs as D
import _render_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
ENTRY = 'frtm_render_frames_u8'
FRTM_ERR_ARG = -1


def test_abi_declares_exports_and_binds_the_entry_point():
    from frtm_vos_amd import _hip, build, ops
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+%s\s*\(' % ENTRY, hdr) and hasattr(_hip.lib(), ENTRY)
    res, args = _hip.SIGNATURES[ENTRY]
    assert res is _hip.I and len(args) == 4                            # two tables, n, stream
    assert 'frame_render.hip' in build.SOURCES
    macros = {k: int(v) for k, v in re.findall(r'#define\s+FRTM_RENDER_(\w+)\s+(\d+)', hdr)}
    assert macros == dict(RGB=ops.RENDER_FORMATS['rgb'], NV12=ops.RENDER_FORMATS['nv12'], LABELS=ops.RENDER_ANSWERS['labels'],
                          MASKS=ops.RENDER_ANSWERS['masks'], ROW_WORDS=ops.RENDER_ROW_WORDS)
    frame = {k.lower(): int(v) for k, v in re.findall(r'#define\s+FRTM_FRAME_(\w+)\s+(\d+)', hdr)}
    assert frame == dict(rgb=0, nv12_bt601=1, nv12_bt601_full=2, nv12_bt709=3, nv12_bt709_full=4) == ops.FRAME_FORMATS      # unchanged
    assert {ops.FRAME_FORMATS[name]: v for name, v in R.FORWARD.items()} == ops.RENDER_YUV
    for name, row in R.FORWARD.items():                                # the header documents the table
        assert re.search(r'\s+'.join(str(v) for v in row), open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read()), name


# ---- refusals of the C entry: addresses that are never followed -----------------------------------------------------------------------
SRC, DST, ANS, LUT, STY = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
KEYS = ['format', 'h', 'w', 'src', 'src_bytes', 'src_pitch', 'src_uv', 'dst', 'dst_bytes', 'dst_pitch', 'dst_uv', 'form', 'ans', 'ans_bytes', 'K',
        'lut', 'style', 'soft', 'edge', 'zero']


def _row(**kw):
    """A valid row: a 7 x 13 NV12 surface of pitch 16 and coded height 10 (16 * 10 + 16 * 4 = 224 bytes) with a K = 3 stack."""
    row = dict(format=1, h=7, w=13, src=SRC, src_bytes=224, src_pitch=16, src_uv=160, dst=DST, dst_bytes=224, dst_pitch=16, dst_uv=160, form=1,
               ans=ANS, ans_bytes=4 * 3 * 7 * 13, K=3, lut=LUT, style=STY, soft=0, edge=-1, zero=0)
    row.update(kw)
    return [row[k] for k in KEYS]


def _call(rows, n=None, host=True, dev=True):
    from frtm_vos_amd import _hip
    L = _hip.lib()
    t = (ctypes.c_longlong * (20 * len(rows)))(*[int(v) for r in rows for v in r])
    rc = L.frtm_render_frames_u8(ctypes.addressof(t) if host else None, ctypes.addressof(t) if dev else None, len(rows) if n is None else n, None)
    return rc, L.frtm_last_error().decode()


LABELS = dict(form=0, ans_bytes=7 * 13, K=0, lut=0)
REFUSED = [
    (dict(K=0), 'stack of 0 planes'), (dict(K=17, ans_bytes=4 * 17 * 7 * 13), 'stack of 17 planes'),
    (dict(h=0), 'size 0 x 13'), (dict(w=0), 'size 7 x 0'), (dict(h=16385), 'size 16385 x 13'), (dict(w=16385, src_pitch=16386, dst_pitch=16386), 'size 7 x 16385'),
    (dict(src_pitch=13), 'source pitch 13, below its 14-byte chroma row'), (dict(dst_pitch=13), 'destination pitch 13, below its 14-byte chroma row'),
    (dict(dst_bytes=223), 'destination .* leaves its 223-byte buffer'), (dict(src_bytes=223), 'source .* leaves its 223-byte buffer'),
    (dict(format=0, src_bytes=3 * 7 * 13, dst_bytes=3 * 7 * 13 - 1), 'destination .* leaves its 272-byte buffer'),
    (dict(src_uv=16 * 7 - 1), 'source .* leaves'), (dict(dst_uv=-1), 'destination .* leaves'),
    (dict(ans_bytes=4 * 3 * 7 * 13 - 1), 'answer leaves its 1091-byte buffer'), (dict(LABELS, ans_bytes=90), 'answer leaves its 90-byte buffer'),
    (dict(dst=SRC + 1), 'overlaps its source in part'), (dict(dst=SRC + 223), 'overlaps its source in part'), (dict(dst=SRC - 223), 'overlaps its source in part'),
    (dict(dst=SRC, dst_pitch=32, dst_uv=320, dst_bytes=448), 'overlaps its source in part'),       # the same address, another layout
    (dict(ans=DST + 100), 'overlaps its answer'),
    (dict(LABELS, soft=1), 'soft blend of a label map'), (dict(soft=1, edge=9), 'no edge under soft'), (dict(soft=2), 'soft 2'),
    (dict(edge=256), 'edge_alpha 256'), (dict(edge=-2), 'edge_alpha -2'),
    (dict(src=0), 'null address'), (dict(dst=0), 'null address'), (dict(ans=0), 'null address'), (dict(style=0), 'null address'), (dict(lut=0), 'null address'),
    (dict(format=2), 'format 2'), (dict(form=2), 'answer form 2'), (dict(zero=1), 'last word 1'),
    (dict(ans=ANS + 2), 'not 4-byte aligned'), (dict(src_bytes=1 << 47), 'not a size'), (dict(src_pitch=1 << 62, src_bytes=1 << 46), 'source .* leaves'),
]


@pytest.mark.parametrize('change,message', REFUSED, ids=[m for _, m in REFUSED])
def test_bad_rows_are_refused_before_any_launch(change, message):
    """The checks read the host table alone: nothing follows an address, so no device is needed to get FRTM_ERR_ARG -- and a launch
    through these addresses would not return at all."""
    rc, msg = _call([_row(), _row(**change)])
    assert rc == FRTM_ERR_ARG and ENTRY in msg and 'frame 1' in msg and re.search(message, msg), msg


def test_bad_calls_are_refused_before_any_launch():
    for kw, message in ((dict(n=0), 'n = 0'), (dict(n=-1), 'n = -1'), (dict(n=65536), 'n = 65536'), (dict(host=False), 'null table'), (dict(dev=False), 'null table')):
        rc, msg = _call([_row()], **kw)
        assert rc == FRTM_ERR_ARG and ENTRY in msg and message in msg, (kw, msg)


# ---- the reference against exact arithmetic --------------------------------------------------------------------------------------------
def test_mix_is_exact_rounding_for_every_input():
    """round(s + (c - s) a / 255), half up, in integers: floor((2 (255 s + (c - s) a) + 255) / 510), for all 256^3 (s, c, a)."""
    s, c = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing='ij')
    worst = 0
    for a in range(256):
        exact = (2 * (255 * s + (c - s) * a) + 255) // 510
        worst = max(worst, int(np.abs(R.mix(s, c, a) - exact).max()))
    assert worst == 0
    assert int(R.mix(7, 200, 0)) == 7 and int(R.mix(7, 200, 255)) == 200 and int(R.mix(0, 255, 128)) == 128 and int(R.mix(255, 0, 128)) == 127


@pytest.mark.parametrize('name', D.NV12)
def test_forward_table_is_within_one_of_the_fp64_matrix(name):
    y0, m = R.real_forward(name)
    assert [y0] + [int(round(65536 * c)) for c in m.reshape(-1)] == list(R.FORWARD[name])
    g = np.linspace(0, 255, 53).round().astype(np.int64)
    lattice = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    rgb = np.concatenate([lattice, np.random.default_rng(3).integers(0, 256, (200000, 3))])
    got, want = R.rgb_to_yuv(rgb, name).astype(np.int64), R.rgb_to_yuv_real(rgb, name).astype(np.int64)
    diff = np.abs(got - want)
    print('%s: max difference %d, differing share %.2e over %d values' % (name, int(diff.max()), float((diff != 0).mean()), diff.size))
    assert int(diff.max()) <= 1
    assert got[0].tolist() == [y0, 128, 128] and got[lattice.shape[0] - 1].tolist() == [255 if y0 == 0 else 235, 128, 128]      # black and white
    from frtm_vos_amd import ops
    assert np.array_equal(ops.rgb_to_yuv_u8(torch.from_numpy(rgb), ops.FRAME_FORMATS[name]).numpy(), R.rgb_to_yuv(rgb, name))


def test_reference_rules_on_hand_made_pixels():
    lut = np.array([0, 5, 9], dtype=np.uint8)
    stack = np.zeros((3, 1, 8), dtype=np.float32)
    stack[1, 0, :6] = [0.5, 0.50001, 0.75, 1.5, -0.25, np.nan]
    stack[2, 0, 2] = 0.75                                              # two equal planes: the first wins
    stack[2, 0, 5] = 0.625                                             # a NaN never wins
    stack[:, 0, 6] = [0.9, 0.75, 0.8]                                  # the background plane is the largest
    assert R.decode_labels(stack, lut)[0].tolist() == [0, 5, 5, 5, 0, 9, 0, 0]
    m, ks = R.soft_terms(stack)
    assert m[0].tolist() == [0.5, np.float32(0.50001), 0.75, 1.0, 0.0, 0.625, np.float32(0.8), 0.0] and ks[0].tolist() == [1, 1, 1, 1, 2, 2, 2, 1]
    nan_only = np.full((2, 1, 1), np.nan, dtype=np.float32)
    assert R.soft_terms(nan_only)[0].tolist() == [[0.0]] and R.soft_terms(stack[:1])[0].max() == 0
    labels = np.array([[1, 1, 0], [1, 2, 0], [0, 0, 0]], dtype=np.uint8)
    assert R.edge_mask(labels, 0).astype(int).tolist() == [[0, 1, 0], [1, 1, 0], [0, 0, 0]]      # the border makes no edge; the background has none
    table = R.style_table(np.arange(768).reshape(256, 3) % 256, alpha=255)
    s = np.full((3, 3, 3), 77, dtype=np.uint8)
    out = R.render_444(s, labels, None, table)
    assert out[:, 0, 0].tolist() == [3, 4, 5] and out[:, 1, 1].tolist() == [6, 7, 8] and out[:, 2, 2].tolist() == [77, 77, 77]
    # soft with m in {0, 1} is the hard rule
    hard = np.where(np.arange(3)[:, None, None] == np.array([[0, 1, 2, 1]])[None], np.float32(1), np.float32(0)).astype(np.float32)
    s4 = np.random.default_rng(0).integers(0, 256, (3, 1, 4), dtype=np.uint8)
    t2 = R.style_table(np.random.default_rng(1).integers(0, 256, (256, 3)), alpha=99, background=(1, 2, 3, 40))
    assert np.array_equal(R.render_444(s4, hard, lut, t2, soft=True), R.render_444(s4, hard, lut, t2))
    # chroma: a block in which nothing changes keeps its bytes; odd sizes average the pixels the picture has
    buf, uv = D.random_surface(np.random.default_rng(2), 3, 5, 8, 4, fill=200)
    assert np.array_equal(R.store_nv12(buf, R.nv12_444(buf, 3, 5, 8, uv), 8, uv), buf)
    yuv = R.nv12_444(buf, 3, 5, 8, uv).copy()
    yuv[1, 0, 0], yuv[1, 0, 1], yuv[1, 1, 0], yuv[1, 1, 1] = 1, 2, 2, 1  # sum 6: (6 + 2) // 4 = 2
    yuv[2, 2, 4] = 9                                                    # the corner block has one pixel
    got = R.store_nv12(buf, yuv, 8, uv)
    assert got[uv] == 2 and got[uv + 8 + 5] == 9 and int((got != buf).sum()) <= 3 + 2 and np.array_equal(got[~D.sample_mask(3, 5, 8, 4)], buf[~D.sample_mask(3, 5, 8, 4)])


# ---- RenderStyle -----------------------------------------------------------------------------------------------------------------------
def test_render_style_tables():
    from frtm_vos_amd import ops
    from frtm_vos_amd.lib.image import davis_palette
    st = ops.RenderStyle()
    assert st.table.dtype == torch.uint8 and tuple(st.table.shape) == (256, 4) and st.soft is False and st.edge_alpha is None
    assert np.array_equal(st.table.numpy(), R.style_table(davis_palette, 128))
    assert st.table[0].tolist() == [0, 0, 0, 0] and st.table[1].tolist() == [128, 0, 0, 128] and st.table_for(0) is st.table
    pal = np.random.default_rng(4).integers(0, 256, (256, 3), dtype=np.uint8)
    alpha = np.random.default_rng(5).integers(0, 256, 256)
    for a in (alpha, alpha.tolist(), torch.from_numpy(alpha), torch.from_numpy(alpha).to(torch.uint8)):
        assert np.array_equal(ops.RenderStyle(pal, alpha=a).table.numpy(), R.style_table(pal, alpha))       # a_0 = 0 whatever the vector holds
    st = ops.RenderStyle(torch.from_numpy(pal), alpha=0, background=(9, 8, 7, 255), edge_alpha=255)
    assert np.array_equal(st.table.numpy(), R.style_table(pal, 0, (9, 8, 7, 255))) and st.edge_alpha == 255 and st.table[0].tolist() == [9, 8, 7, 255]
    for name in D.NV12:
        t = st.table_for(ops.FRAME_FORMATS[name])
        assert np.array_equal(t.numpy(), R.style_table(pal, 0, (9, 8, 7, 255), name=name)) and np.array_equal(t[:, 3].numpy(), st.table[:, 3].numpy())
    assert ops.RenderStyle(soft=True).soft is True and ops.default_render_style() is ops.default_render_style()


def test_render_style_refusals():
    from frtm_vos_amd import ops
    pal = np.zeros((256, 3), dtype=np.uint8)
    for bad in (pal[:255], pal[:, :2], np.zeros((256, 3, 1), dtype=np.uint8)):
        with pytest.raises(ValueError, match=r'\(256, 3\)'):
            ops.RenderStyle(bad)
    for bad in (pal.astype(np.float32), pal.astype(np.int64), pal.tolist(), 'davis'):
        with pytest.raises(TypeError, match='palette'):
            ops.RenderStyle(bad)
    for bad in (-1, 256, [1] * 255, np.full(256, 256), np.full(256, -1), np.zeros((256, 1), dtype=np.int64)):
        with pytest.raises(ValueError, match='alpha'):
            ops.RenderStyle(pal, alpha=bad)
    for bad in (0.5, True, None, '128', np.full(256, 0.5)):
        with pytest.raises(TypeError, match='alpha'):
            ops.RenderStyle(pal, alpha=bad)
    for bad in ((1, 2, 3), (1, 2, 3, 4, 5)):
        with pytest.raises(ValueError, match='background'):
            ops.RenderStyle(pal, background=bad)
    with pytest.raises(ValueError, match='background'):
        ops.RenderStyle(pal, background=(1, 2, 3, 256))
    for bad in (7, 'red', (1, 2, 3, 0.5)):
        with pytest.raises(TypeError, match='background'):
            ops.RenderStyle(pal, background=bad)
    with pytest.raises(ValueError, match='edge_alpha'):
        ops.RenderStyle(pal, edge_alpha=300)
    with pytest.raises(TypeError, match='edge_alpha'):
        ops.RenderStyle(pal, edge_alpha=0.5)
    with pytest.raises(TypeError, match='soft'):
        ops.RenderStyle(pal, soft=1)
    with pytest.raises(ValueError, match='soft has no edges'):
        ops.RenderStyle(pal, soft=True, edge_alpha=10)


def test_render_frames_refuses_before_any_launch():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from frtm_vos_amd import ops
    st = ops.RenderStyle()
    cpu = torch.zeros(3, 4, 6, dtype=torch.uint8)
    with pytest.raises(TypeError, match='RenderStyle'):
        ops.render_frames([cpu], [cpu[0]], None)
    with pytest.raises(ValueError, match='0 frames'):
        ops.render_frames([], [], st)
    with pytest.raises(ValueError, match='1 frames, 2 answers'):
        ops.render_frames([cpu], [cpu[0], cpu[0]], st)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.render_frames([cpu], [cpu[0]], st)
    with pytest.raises(TypeError, match=r'\(3, H, W\) uint8'):
        ops.render_frames([cpu.float()], [cpu[0]], st)
    with pytest.raises(TypeError, match=r'\(3, H, W\) uint8'):
        ops.render_frames([cpu[:2]], [cpu[0]], st)
    with FakeTensorMode():
        frame = torch.empty(3, 4, 6, dtype=torch.uint8, device='cuda')
        labels = torch.empty(4, 6, dtype=torch.uint8, device='cuda')
        stack = torch.empty(2, 4, 6, device='cuda')
        lut = torch.empty(2, dtype=torch.uint8, device='cuda')
        stack17 = torch.empty(17, 4, 6, device='cuda')
        surface = torch.empty(ops.DecoderFrame.layout(4, 6)[2], dtype=torch.uint8, device='cuda')
    with pytest.raises(TypeError, match='label map or a'):
        ops.render_frames([frame], [labels.float()], st)
    with pytest.raises(TypeError, match='label map or a'):
        ops.render_frames([frame], [stack.double()], st)
    with pytest.raises(ValueError, match='answer 0 has size'):
        ops.render_frames([frame], [labels[:3]], st)
    with pytest.raises(TypeError, match=r'needs luts\[0\]'):
        ops.render_frames([frame], [stack], st)
    with pytest.raises(TypeError, match=r'needs luts\[0\]'):
        ops.render_frames([frame], [stack], st, luts=[lut[:1]])
    with pytest.raises(ValueError, match='17 planes'):
        ops.render_frames([frame], [stack17], st, luts=[lut])
    with pytest.raises(ValueError, match='soft style needs the mask stack'):
        ops.render_frames([frame], [labels], ops.RenderStyle(soft=True))
    with pytest.raises(ValueError, match='out 0 is an NV12 surface'):
        ops.render_frames([frame], [labels], st, out=[ops.DecoderFrame(surface, 4, 6)])
    with pytest.raises(ValueError, match='out 0 is planar RGB'):
        ops.render_frames([ops.DecoderFrame(surface, 4, 6)], [labels], st, out=[frame])
    with pytest.raises(ValueError, match='out 0'):
        ops.render_frames([ops.DecoderFrame(surface, 4, 6)], [labels], st, out=[ops.DecoderFrame(surface, 4, 6, matrix='bt601')])


def test_tracker_and_pool_have_the_surface():
    import inspect
    from frtm_vos_amd.model.stream_pool import StreamPool
    from frtm_vos_amd.model.tracker import Tracker
    assert list(inspect.signature(Tracker.render).parameters) == ['self', 'image', 'style', 'out']
    assert list(inspect.signature(StreamPool.render).parameters) == ['self', 'frames', 'style', 'out']
    import types
    state = types.SimpleNamespace(native_labels=None, current_masks=None, targets={})      # a tracker before its first frame
    frame = torch.zeros(3, 4, 6, dtype=torch.uint8)
    with pytest.raises(ValueError, match='nothing was tracked'):
        Tracker.render_answer(state, frame, None)
    state.current_masks = torch.zeros(1, 8, 6)
    with pytest.raises(ValueError, match=r'size \(4, 6\) \(the last step answered at \(8, 6\)\)'):
        Tracker.render_answer(state, frame, None)
    with pytest.raises(ValueError, match=r'answered at \(2, 3\)'):
        Tracker.render_answer(state, frame, torch.zeros(1, 2, 3, dtype=torch.uint8))
    labels = torch.ones(1, 4, 6, dtype=torch.uint8)
    answer, lut = Tracker.render_answer(state, frame, labels)
    assert lut is None and tuple(answer.shape) == (4, 6) and answer.data_ptr() == labels.data_ptr()


# ---- the kernel's budget ---------------------------------------------------------------------------------------------------------------
def test_kernel_uses_no_scratch_and_spills_nothing():
    assert os.path.exists(HIPCC), 'hipcc is needed (the build needs it as well)'
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'frame_render.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'frame_render.hip')], check=True, capture_output=True, cwd=d)
        isa = open(out).read()
    kernel = 'k_render_frames'
    meta = isa[isa.index('amdhsa.kernels:'):]
    blocks = [b for b in meta.split('\n  - ') if re.search(r'\.name:\s+_Z%d%s[A-Z]' % (len(kernel), kernel), b)]
    assert len(blocks) == 1
    field = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, blocks[0]).group(1))
    print('%s: %d VGPRs, %d SGPRs, %d bytes of LDS' % (kernel, field('vgpr_count'), field('sgpr_count'), field('group_segment_fixed_size')))
    assert field('vgpr_spill_count') == 0 and field('sgpr_spill_count') == 0 and field('private_segment_fixed_size') == 0
    assert 0 < field('group_segment_fixed_size') <= 16 * 1024          # four workgroups and more per CU
    assert not re.search(r'\.uses_dynamic_stack:\s+true', blocks[0])
