"""The renderer on the GPU: frtm_render_frames_u8 (csrc/frame_render.hip) through ops.render_frames, Tracker.render and StreamPool.render.

Every output byte is an integer function of the inputs, so everything is compared BYTE FOR BYTE with the numpy statement of
tests/_render_refs.py (which tests/test_frame_render.py holds to exact arithmetic); there is no tolerance anywhere in this file.  The whole
destination buffer is compared, sentinel bytes in front of it and behind it included: a byte of padding that changed fails the case.  NV12
surfaces start at an odd byte address; every case runs twice with different bytes in the source's padding, and the picture samples of the
two results must agree."""
import numpy as np
import pytest
import torch

import _decoder_refs as D
import _render_refs as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = 'cuda:0'
LEAD, TAIL = 1, 3                                 # sentinel bytes around every buffer; LEAD odd: the surface starts at an odd address

# (h, w, pitch or None: 2 ceil(w / 2), coded height or None: h)
SIZES = [(1, 1, None, None), (2, 2, None, None), (1, 7, None, None), (7, 13, 16, 10), (16, 64, None, None), (17, 65, None, None), (33, 130, 192, None)]
ANSWERS = [('labels', 'hard'), ('labels', 'edge')] + [(K, mode) for K in (1, 3, 16) for mode in ('hard', 'edge', 'soft')]
ALL = [(size, fmt, ans, mode, place) for size in SIZES for fmt in ('rgb', 'nv12') for ans, mode in ANSWERS for place in ('out', 'in')]
CASES = ALL[::5]                                  # 62 of the 308; 5 is coprime to the 44 (format, answer, mode, place) combinations: all occur


def test_the_pruned_matrix_keeps_every_size_format_answer_and_mode():
    assert 55 <= len(CASES) <= 65
    assert {(c[0], c[1]) for c in CASES} == {(s, f) for s in SIZES for f in ('rgb', 'nv12')}
    assert {c[1:] for c in CASES} == {a[1:] for a in ALL}


def _buffer(payload, fill):
    """``payload`` (flat uint8 numpy) on the device with LEAD + TAIL sentinel bytes around it -> (whole tensor, the view of the payload)."""
    big = np.full(LEAD + payload.size + TAIL, fill, dtype=np.uint8)
    big[LEAD:LEAD + payload.size] = payload
    t = torch.from_numpy(big).to(DEV)
    view = t[LEAD:LEAD + payload.size]
    assert view.data_ptr() % 2 == 1
    return t, view


def _pattern(n, seed):
    return ((np.arange(n) * 7 + seed) % 251).astype(np.uint8)


def _style(rng, ci, mode):
    from frtm_vos_amd import ops
    pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    alpha = rng.integers(0, 256, 256)
    bg = None if ci % 2 else tuple(int(v) for v in rng.integers(0, 256, 4))
    edge = (255, 200, 0)[ci % 3] if mode == 'edge' else None
    return ops.RenderStyle(pal, alpha=alpha, background=bg, edge_alpha=edge, soft=mode == 'soft'), (pal, alpha, bg, edge)


def _answer(rng, ans, h, w, ci):
    """-> (numpy answer, numpy lut or None)."""
    if ans == 'labels':
        return R.blob_labels(rng, h, w, [0, 3, 200, 255]), None
    lut = np.concatenate([[0 if ci % 2 == 0 else 7], rng.permutation(np.arange(8, 250))[:ans - 1]]).astype(np.uint8)
    return R.hand_placed(R.merged_stack(rng, ans, h, w)), lut


def _run_case(ci, case, pad_fill):
    """One case with ``pad_fill`` in the source's padding -> (whole destination buffer after the call, its expected bytes, sample mask of
    the destination inside the whole buffer)."""
    from frtm_vos_amd import ops
    (h, w, pitch, coded), fmt, ans, mode, place = case
    rng = np.random.default_rng(100 + ci)
    style, (pal, alpha, bg, edge) = _style(rng, ci, mode)
    answer, lut = _answer(rng, ans, h, w, ci)
    ans_t = torch.from_numpy(answer).to(DEV)
    luts = [None if lut is None else torch.from_numpy(lut).to(DEV)]
    soft = mode == 'soft'
    if fmt == 'rgb':
        src = rng.integers(0, 256, 3 * h * w, dtype=np.uint8)
        s_whole, s_view = _buffer(src, 0x5A)
        frame = s_view.view(3, h, w)
        want_px = R.render_444(src.reshape(3, h, w), answer, lut, R.style_table(pal, alpha, bg), soft, edge).reshape(-1)
        if place == 'in':
            d_whole, out = s_whole, [frame]
        else:
            d_whole, d_view = _buffer(_pattern(3 * h * w, ci), 0xC3)
            out = [d_view.view(3, h, w)]
        initial = d_whole.cpu().numpy().copy()
        got = ops.render_frames([frame], [ans_t], style, luts=luts, out=out)
        assert got[0] is out[0]
        want = initial.copy()
        want[LEAD:LEAD + want_px.size] = want_px
        mask = np.zeros(want.size, dtype=bool)
        mask[LEAD:LEAD + want_px.size] = True
        return d_whole.cpu().numpy(), want, mask
    name = D.NV12[ci % 4]
    pitch = 2 * ((w + 1) // 2) if pitch is None else pitch
    coded = h if coded is None else coded
    src, uv = D.random_surface(rng, h, w, pitch, coded, fill=pad_fill)
    s_whole, s_view = _buffer(src, 0x5A)
    matrix, full = name.split('_')[1], name.endswith('_full')
    frame = ops.DecoderFrame(s_view, h, w, pitch=pitch, uv_offset=uv, matrix=matrix, full_range=full)
    table = R.style_table(pal, alpha, bg, name=name)
    if place == 'in':
        d_whole, out, dpitch, dcoded, duv = s_whole, [frame], pitch, coded, uv
    else:
        dpitch, dcoded = pitch + 2 * (ci % 3), coded + ci % 2          # the destination's own layout
        duv = dpitch * dcoded
        d_whole, d_view = _buffer(_pattern(D.surface_bytes(h, w, dpitch, dcoded), ci), 0xC3)
        out = [ops.DecoderFrame(d_view, h, w, pitch=dpitch, uv_offset=duv, matrix=matrix, full_range=full)]
    initial = d_whole.cpu().numpy().copy()
    got = ops.render_frames([frame], [ans_t], style, luts=luts, out=out)
    assert got[0] is out[0]
    n = D.surface_bytes(h, w, dpitch, dcoded)
    want = initial.copy()
    want[LEAD:LEAD + n] = R.render_nv12(src, h, w, pitch, uv, initial[LEAD:LEAD + n], dpitch, duv, answer, lut, table, soft, edge)
    mask = np.zeros(want.size, dtype=bool)
    mask[LEAD:LEAD + n] = D.sample_mask(h, w, dpitch, dcoded)
    return d_whole.cpu().numpy(), want, mask


@pytest.fixture(scope='module')
def matrix_results():
    return [(_run_case(ci, case, 0x11), _run_case(ci, case, 0xEE)) for ci, case in enumerate(CASES)]


def _case_id(c):
    (h, w, pitch, coded), fmt, ans, mode, place = c
    return '%dx%d-%s-%s-%s-%s' % (h, w, fmt, ans if ans == 'labels' else 'K%d' % ans, mode, place)


@pytest.mark.parametrize('ci', range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_render_equals_the_reference_byte_for_byte(matrix_results, ci):
    (got, want, mask), (got2, want2, _) = matrix_results[ci]
    assert got.dtype == np.uint8 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, 'first differing bytes at %r (sample: %r): got %r, want %r' % (bad[:8].tolist(), mask[bad[:8]].tolist(), got[bad[:8]].tolist(),
                                                                                      want[bad[:8]].tolist())
    assert np.array_equal(got2, want2)                                  # the second run, other bytes in the source's padding
    assert np.array_equal(got2[mask], got[mask])                        # ... gives the same picture: the padding is not read
    assert int((got[mask] != 0).sum()) > 0 or mask.sum() < 8


def test_the_matrix_meets_the_hand_placed_pixels():
    """The stacks of the matrix hold the pixels the decode can get wrong; the reference sees them as the definition says."""
    stack = R.hand_placed(R.merged_stack(np.random.default_rng(0), 3, 16, 64))
    lut = np.array([0, 5, 9], dtype=np.uint8)
    assert R.decode_labels(stack, lut)[0, :7].tolist() == [0, 5, 0, 0, 5, 9, 0]
    m, ks = R.soft_terms(stack)
    assert m[0, :7].tolist() == [0.5, 1.0, 0.0, 0.0, 0.75, 0.625, np.float32(0.8)] and ks[0, :7].tolist() == [1, 1, 2, 2, 1, 2, 2]


# ---- single launches through the wrappers ---------------------------------------------------------------------------------------------
def _rgb_frame(rng, h, w):
    src = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    return src, torch.from_numpy(src).to(DEV)


def _nv12_frame(rng, h, w, pitch, coded, name, fill=0x33):
    from frtm_vos_amd import ops
    src, uv = D.random_surface(rng, h, w, pitch, coded, fill=fill)
    frame = ops.DecoderFrame(torch.from_numpy(src).to(DEV), h, w, pitch=pitch, uv_offset=uv, matrix=name.split('_')[1], full_range=name.endswith('_full'))
    return src, uv, frame


def _edge_patterns():
    h, w = 40, 140
    y, x = np.mgrid[:h, :w]
    checker = np.where((y + x) % 2 == 0, 4, 9).astype(np.uint8)
    checker[:, 100:] = np.where((y[:, 100:] // 3 + x[:, 100:] // 5) % 2 == 0, 0, 6)
    frame_obj = np.full((h, w), 12, dtype=np.uint8)                     # an object that touches all four borders, a hole of background inside
    frame_obj[5:35, 7:120] = 0
    tiles = np.zeros((h, w), dtype=np.uint8)                            # boundaries along columns 63|64 and rows 15|16: the tile borders
    tiles[:16, :64], tiles[16:, 64:] = 21, 22
    return [('checkerboard', checker), ('touches_the_borders', frame_obj), ('along_the_tile_borders', tiles)]


@pytest.mark.parametrize('fmt', ['rgb', 'nv12'])
@pytest.mark.parametrize('which', range(3), ids=[n for n, _ in _edge_patterns()])
def test_edge_geometry(which, fmt):
    from frtm_vos_amd import ops
    _, labels = _edge_patterns()[which]
    h, w = labels.shape
    rng = np.random.default_rng(40 + which)
    pal, alpha = rng.integers(0, 256, (256, 3), dtype=np.uint8), rng.integers(0, 200, 256)
    style = ops.RenderStyle(pal, alpha=alpha, edge_alpha=255)
    edges = R.edge_mask(labels, 0)
    assert edges.any() and not edges.all()
    if which == 1:
        assert not edges[0].any() and not edges[:, 0].any() and not edges[-1].any() and not edges[:, -1].any() and edges[4, 7:120].all()
    if which == 2:
        assert edges[15, :64].all() and edges[16, 64:].all() and edges[:16, 63].all() and edges[16:, 64].all() and not edges[16, :63].any()
    # the same map as a stack: plane k holds object k's pixels at 0.9
    ids = sorted(set(labels.reshape(-1).tolist()) | {0})
    lut = np.array(ids, dtype=np.uint8)
    stack = np.stack([np.where(labels == i, np.float32(0.9), np.float32(0)) for i in ids]).astype(np.float32)
    answers = [torch.from_numpy(labels).to(DEV), torch.from_numpy(stack).to(DEV)]
    luts = [None, torch.from_numpy(lut).to(DEV)]
    if fmt == 'rgb':
        src, frame = _rgb_frame(rng, h, w)
        want = R.render_444(src, labels, None, R.style_table(pal, alpha), edge_alpha=255)
        got = ops.render_frames([frame, frame], answers, style, luts=luts)
        assert np.array_equal(got[0].cpu().numpy(), want) and np.array_equal(got[1].cpu().numpy(), want)
        assert np.array_equal(got[0].cpu().numpy()[:, edges], pal[labels[edges]].T)          # alpha 255 on the edges: the palette itself
    else:
        name = D.NV12[which]
        src, uv, frame = _nv12_frame(rng, h, w, 144, 48, name)
        want = R.render_nv12(src, h, w, 144, uv, src, 144, uv, labels, None, R.style_table(pal, alpha, name=name), edge_alpha=255)
        got = ops.render_frames([frame, frame], answers, style, luts=luts)
        assert np.array_equal(got[0].data.cpu().numpy()[D.sample_mask(h, w, 144, 48)], want[D.sample_mask(h, w, 144, 48)])
        assert torch.equal(got[0].data[torch.from_numpy(D.sample_mask(h, w, 144, 48)).to(DEV)], got[1].data[torch.from_numpy(D.sample_mask(h, w, 144, 48)).to(DEV)])
        assert (got[0].pitch, got[0].uv_offset, got[0].format) == (frame.pitch, frame.uv_offset, frame.format)


def test_identities():
    from frtm_vos_amd import ops
    rng = np.random.default_rng(50)
    h, w = 19, 37
    labels = R.blob_labels(rng, h, w, [0, 1, 2, 77])
    labels_t = torch.from_numpy(labels).to(DEV)
    pal = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    src, frame = _rgb_frame(rng, h, w)
    name = 'nv12_bt601'
    nsrc, uv, nframe = _nv12_frame(rng, h, w, 48, 24, name)
    mask = D.sample_mask(h, w, 48, 24)
    # (i) every alpha 0: the destination equals the source on picture samples, out of place and in place
    zero = ops.RenderStyle(pal, alpha=0)
    for edge in (None, 0):
        st = zero if edge is None else ops.RenderStyle(pal, alpha=0, edge_alpha=0)
        out = ops.render_frames([frame, nframe], [labels_t, labels_t], st)
        assert np.array_equal(out[0].cpu().numpy(), src) and np.array_equal(out[1].data.cpu().numpy()[mask], nsrc[mask])
    copy, ncopy = frame.clone(), ops.DecoderFrame(nframe.data.clone(), h, w, pitch=48, uv_offset=uv, matrix='bt601')
    same = ops.render_frames([copy, ncopy], [labels_t, labels_t], zero, out=[copy, ncopy])
    assert same[0] is copy and np.array_equal(copy.cpu().numpy(), src) and np.array_equal(ncopy.data.cpu().numpy(), nsrc)
    # (ii) alpha 255 for every id, the background included: the planes are the palette entries (NV12: their converted bytes)
    full = ops.RenderStyle(pal, alpha=255, background=tuple(pal[0].tolist()) + (255,))
    out = ops.render_frames([frame, nframe], [labels_t, labels_t], full)
    assert np.array_equal(out[0].cpu().numpy(), pal[labels].transpose(2, 0, 1))
    yuv = R.rgb_to_yuv(pal, name)[labels].transpose(2, 0, 1)
    assert np.array_equal(out[1].data.cpu().numpy()[mask], R.store_nv12(nsrc, yuv, 48, uv)[mask])
    # (iii) the hard rule on a stack = the hard rule on the labels ops.masks_to_native makes of that stack on equal sizes
    K = 5
    stack = R.hand_placed(R.merged_stack(rng, K, h, w))
    lut = torch.tensor([0, 9, 8, 250, 3], dtype=torch.uint8, device=DEV)
    stack_t = torch.from_numpy(stack).to(DEV)
    table = ops.NativeTable.packed((h, w), [(K, h, w)], DEV, soft=False)
    native = torch.zeros(h * w, dtype=torch.uint8, device=DEV)
    ops.masks_to_native(stack_t, table, native, lut)
    assert np.array_equal(native.cpu().numpy().reshape(h, w), R.decode_labels(stack, lut.cpu().numpy()))
    st = ops.RenderStyle(pal, alpha=rng.integers(0, 256, 256), edge_alpha=222)
    a = ops.render_frames([frame, nframe], [stack_t, stack_t], st, luts=[lut, lut])
    b = ops.render_frames([frame, nframe], [native.view(h, w), native.view(h, w)], st)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].data[torch.from_numpy(mask).to(DEV)], b[1].data[torch.from_numpy(mask).to(DEV)])
    assert not torch.equal(a[0], frame)


def _five(rng):
    """Five frames of different sizes, formats and answer forms -> per frame (frame, answer tensor, lut tensor or None, sentinel out)."""
    from frtm_vos_amd import ops
    rows = []
    for k, (h, w, fmt, ans) in enumerate([(9, 70, 'rgb', 'labels'), (21, 33, 'nv12_bt709', 3), (5, 5, 'nv12_bt601_full', 'labels'), (35, 129, 'rgb', 16),
                                          (18, 64, 'nv12_bt601', 1)]):
        answer, lut = _answer(rng, ans, h, w, k)
        if fmt == 'rgb':
            frame = _rgb_frame(rng, h, w)[1]
            out = torch.full_like(frame, 0x77)
        else:
            pitch, coded = 2 * ((w + 1) // 2) + 4 * k, h + k
            _, uv, frame = _nv12_frame(rng, h, w, pitch, coded, fmt)
            need = ops.DecoderFrame.layout(h, w, pitch + 2, (pitch + 2) * coded)[2]
            out = ops.DecoderFrame(torch.full((need + 5,), 0x77, dtype=torch.uint8, device=DEV), h, w, pitch=pitch + 2, uv_offset=(pitch + 2) * coded,
                                   matrix=frame.matrix, full_range=frame.full_range)
        rows.append((frame, torch.from_numpy(answer).to(DEV), None if lut is None else torch.from_numpy(lut).to(DEV), out))
    return rows


def _bytes_of(f):
    return f.data if hasattr(f, 'data') and not isinstance(f, torch.Tensor) else f


def test_one_launch_for_five_frames_equals_five_launches():
    from frtm_vos_amd import ops
    rows = _five(np.random.default_rng(60))
    style = ops.RenderStyle(alpha=np.arange(256)[::-1].copy(), background=(10, 20, 30, 99), edge_alpha=250)
    frames, answers, luts, outs = (list(v) for v in zip(*rows))
    got = ops.render_frames(frames, answers, style, luts=luts, out=outs)
    assert all(g is o for g, o in zip(got, outs))
    first = [_bytes_of(o).clone() for o in outs]
    kept = len(ops._render_tables)
    ops.render_frames(frames, answers, style, luts=luts, out=outs)       # the same surfaces again: the uploaded table is found, not made
    assert len(ops._render_tables) == kept <= ops.RENDER_TABLES_KEPT and all(torch.equal(_bytes_of(o), b) for o, b in zip(outs, first))
    for k in range(5):
        single = ops.render_frames([frames[k]], [answers[k]], style, luts=[luts[k]])[0]
        if isinstance(single, torch.Tensor):
            assert torch.equal(single, got[k]) and not torch.equal(got[k], torch.full_like(got[k], 0x77))
        else:                                                           # its own layout: compare the pictures
            h, w = frames[k].height, frames[k].width
            a = R.nv12_444(got[k].data.cpu().numpy(), h, w, got[k].pitch, got[k].uv_offset)
            b = R.nv12_444(single.data.cpu().numpy(), h, w, single.pitch, single.uv_offset)
            assert np.array_equal(a, b)
            pad = ~np.pad(D.sample_mask(h, w, got[k].pitch, h + k), (0, got[k].data.numel() - got[k].nbytes_needed))
            assert bool((got[k].data.cpu().numpy()[pad] == 0x77).all())


def test_a_row_that_leaves_its_buffer_raises_and_launches_nothing():
    from frtm_vos_amd import ops
    rows = _five(np.random.default_rng(61))
    frames, answers, luts, outs = (list(v) for v in zip(*rows))
    outs[2].data = outs[2].data[:outs[2].nbytes_needed - 1]             # a surface whose bookkeeping promises one byte too many
    with pytest.raises(RuntimeError, match=r"frtm_render_frames_u8 failed \(-1\).*frame 2's destination .* leaves its"):
        ops.render_frames(frames, answers, ops.RenderStyle(), luts=luts, out=outs)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((_bytes_of(o) == 0x77).all())
    with pytest.raises(RuntimeError, match='overlaps its source in part'):
        whole = torch.zeros(3 * 9 * 70 + 1, dtype=torch.uint8, device=DEV)
        ops.render_frames([whole[:-1].view(3, 9, 70)], [answers[0]], ops.RenderStyle(), out=[whole[1:].view(3, 9, 70)])


# ---- Tracker and StreamPool ------------------------------------------------------------------------------------------------------------
WS = (128, 160)
BIG = (256, 320)


def _params(working_size=None):
    """The configuration of tests/test_decoder_frames_gpu.py: ResNet-18, fast parameters, a short memory."""
    from frtm_vos_amd.evaluate import Parameters
    torch.manual_seed(0)
    kw = {} if working_size is None else dict(working_size=working_size)
    params = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18', feature_batch=8, trunk_lanes=2, **kw)
    params.disc_params.update(memory_size=8, init_iters=(2, 3), update_iters=(3,))
    return params


def _sequence(name, frames, size, n_obj, seed, fmt=None, pitch=None):
    """A synthetic sequence -> [(frame: tensor, or DecoderFrame when ``fmt`` is given, labels, new_objects)]."""
    from frtm_vos_amd import ops
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    seq = SyntheticSequence(name, frames, size, n_obj, seed=seed)
    seq.preload(DEV)
    out = []
    for t, (image, labels, new_objects) in enumerate(seq):
        labels = labels.to(DEV) if torch.is_tensor(labels) else labels
        if fmt is not None:
            buf, uv_off = D.encode_nv12(image.cpu().numpy(), pitch, fmt, coded_h=size[0] + 8, fill=(37 * t) % 256)
            image = ops.DecoderFrame(torch.from_numpy(buf).to(DEV), size[0], size[1], pitch=pitch, uv_offset=uv_off, matrix=fmt.split('_')[1],
                                     full_range=fmt.endswith('_full'))
        out.append((image, labels, new_objects))
    return out


def _reference_of(frame, answer, lut, name, alpha, background=None, edge=None):
    """The reference picture (3, h, w) of an NV12 frame rendered with the DAVIS palette: the replicated Y, U, V of the result."""
    from frtm_vos_amd.lib.image import davis_palette
    h, w = frame.height, frame.width
    buf = frame.data.cpu().numpy()
    table = R.style_table(davis_palette, alpha, background, name=name)
    out = R.render_nv12(buf, h, w, frame.pitch, frame.uv_offset, buf, frame.pitch, frame.uv_offset, answer, lut, table, edge_alpha=edge)
    return R.nv12_444(out, h, w, frame.pitch, frame.uv_offset)


def _picture(f):
    if isinstance(f, torch.Tensor):
        return f.cpu().numpy()
    return R.nv12_444(f.data.cpu().numpy(), f.height, f.width, f.pitch, f.uv_offset)


@pytest.mark.parametrize('working_size', [None, WS], ids=['plain', 'working_size'])
def test_tracker_render_equals_the_reference(working_size):
    from frtm_vos_amd import ops
    fmt = 'nv12_bt601'
    size = BIG if working_size is not None else WS
    seq = _sequence('rt', 3, size, 2, 81, fmt, size[1] + 32)
    trk = _params(working_size).get_model().eval()
    with pytest.raises(ValueError, match='nothing was tracked'):
        trk.render(seq[0][0])
    torch.manual_seed(0)
    trk.initialize(seq[0][0], seq[0][1], seq[0][2])
    trk.current_frame += 1
    for image, _, _ in seq[1:]:
        masks = trk.track(image)
        trk.current_frame += 1
    before = image.data.clone()
    got = trk.render(image)                                             # the default style: the DAVIS palette at half opacity
    assert isinstance(got, ops.DecoderFrame) and got.data.data_ptr() != image.data.data_ptr() and torch.equal(image.data, before)
    if working_size is not None:
        assert trk.native_labels is not None and tuple(trk.native_labels.shape) == (1,) + BIG and tuple(trk.current_masks.shape[-2:]) == WS
        answer, lut = trk.native_labels[0].cpu().numpy(), None
    else:
        assert trk.native_labels is None and masks.data_ptr() == trk.current_masks.data_ptr()
        answer, lut = trk.current_masks.cpu().numpy(), trk._object_lut().cpu().numpy()
    want = _reference_of(image, answer, lut, fmt, 128)
    assert np.array_equal(_picture(got), want)
    ids, counts = np.unique(R.decode_labels(answer, lut) if lut is not None else answer, return_counts=True)
    print('labels of the last answer:', dict(zip(ids.tolist(), counts.tolist())))
    style = ops.RenderStyle(alpha=200, edge_alpha=255, background=(0, 0, 0, 64))
    original = ops.DecoderFrame(before, size[0], size[1], pitch=image.pitch, uv_offset=image.uv_offset, matrix='bt601')
    assert trk.render(image, style, out=image) is image                 # in place
    assert np.array_equal(_picture(image), _reference_of(original, answer, lut, fmt, 200, (0, 0, 0, 64), 255))
    assert not np.array_equal(_picture(image), _picture(original))      # (the dimmed background alone changes the picture)
    pad = torch.from_numpy(~D.sample_mask(size[0], size[1], image.pitch, size[0] + 8)).to(DEV)
    assert torch.equal(image.data[pad], before[pad])                    # the padding of an in-place surface keeps its bytes
    with pytest.raises(ValueError, match='no answer for a frame of size'):
        trk.render(torch.zeros(3, 64, 64, dtype=torch.uint8, device=DEV))


def test_pool_render_is_one_launch_for_all_streams():
    from frtm_vos_amd import ops
    from frtm_vos_amd.lib.image import davis_palette
    streams = [_sequence('pa', 3, WS, 1, 90), _sequence('pb', 3, WS, 2, 91, 'nv12_bt709', 176), _sequence('pc', 3, BIG, 2, 92, 'nv12_bt601_full', BIG[1] + 32)]
    pool = _params().get_stream_pool(max_streams=3, working_size=WS)
    sids = [pool.open() for _ in streams]
    for t in range(3):
        frames = {}
        for sid, seq in zip(sids, streams):
            image, labels, new_objects = seq[t]
            if len(new_objects) > 0:
                torch.manual_seed(0)
                pool.initialize(sid, image, labels, new_objects)
            frames[sid] = image
        out = pool.step(frames)
    assert sorted(out) == sorted(sids) and sids[2] in pool.native_labels and sids[0] not in pool.native_labels
    counters = (pool.trunk_passes, pool.frame_launches, pool.refiner_passes, pool.grouped_launches)
    assert pool.render_launches == 0
    style = ops.RenderStyle(alpha=160, edge_alpha=255)
    got = pool.render(frames, style)
    assert pool.render_launches == 1 and sorted(got) == sorted(sids)
    assert (pool.trunk_passes, pool.frame_launches, pool.refiner_passes, pool.grouped_launches) == counters
    names = [None, 'nv12_bt709', 'nv12_bt601_full']
    for k, sid in enumerate(sids):
        tr = pool.tracker(sid)
        if sid in pool.native_labels:
            answer, lut = pool.native_labels[sid], None
        else:
            answer, lut = tr.current_masks, tr._object_lut()
        single = ops.render_frames([frames[sid]], [answer.contiguous()], style, luts=[lut])[0]
        assert np.array_equal(_picture(got[sid]), _picture(single))
        assert type(got[sid]) is type(frames[sid]) and tuple(got[sid].shape) == tuple(frames[sid].shape)
        want = R.render_444(_picture(frames[sid]), answer.cpu().numpy(), None if lut is None else lut.cpu().numpy(),
                            R.style_table(davis_palette, 160, name=names[k]), edge_alpha=255)
        if names[k] is None:
            assert np.array_equal(_picture(got[sid]), want)
        else:                                                           # the reference's 4:4:4 result, box-subsampled into the frame's layout
            f = frames[sid]
            buf = f.data.cpu().numpy()
            assert np.array_equal(_picture(got[sid]), R.nv12_444(R.store_nv12(buf, want, f.pitch, f.uv_offset), f.height, f.width, f.pitch, f.uv_offset))
    # into the caller's surfaces, and in place
    mine = {sid: (torch.empty_like(f) if isinstance(f, torch.Tensor) else
                  ops.DecoderFrame(torch.empty_like(f.data), f.height, f.width, pitch=f.pitch, uv_offset=f.uv_offset, matrix=f.matrix, full_range=f.full_range))
            for sid, f in frames.items()}
    again = pool.render(frames, style, out=mine)
    assert pool.render_launches == 2 and all(again[sid] is mine[sid] for sid in sids)
    assert all(np.array_equal(_picture(again[sid]), _picture(got[sid])) for sid in sids)
    with pytest.raises(ValueError, match='no answer for a frame of size'):
        pool.render({sids[0]: torch.zeros(3, 64, 64, dtype=torch.uint8, device=DEV)})
    with pytest.raises(KeyError):
        pool.render({12345: frames[sids[0]]})
    for sid in sids:
        pool.close(sid)
