"""Decoder frames on the GPU: frtm_frames_to_rgb_u8 (csrc/frame_formats.hip) and its way through Tracker and StreamPool.

The kernel's reference runs in this library: the numpy statement of the colour formula (tests/_decoder_refs.py), then
ops.resize_frames_u8 -- the fused launch must equal that BIT FOR BIT (it runs the same passes on the same bytes), and at the picture's own
size it must equal the numpy planes themselves.  So that both kernels cannot be wrong together, the same outputs are also held to the fp64
restatement of the resize (tests/_frame_refs.py) under the rule of tests/test_frame_resize_gpu.py: equal to the half-even rounding of the
fp64 value wherever that lies farther than NEAR_TIE from a tie, at most 1 off elsewhere, and the share of outputs inside that band, taken
on the fp64 reference alone, below BAND_CAP for the frames of non-integer ratio that have enough outputs for a share of 1 % to mean
something (at least 500: three of the cases; the tiny shapes are there for their edges, and ratios such as 6 -> 4 with 10 -> 15 put a
twentieth of the outputs ON a tie, like the 68 -> 51 frame of tests/_frame_refs.py, which says nothing about a kernel).

Tracker and pool: a tracker fed DecoderFrames must equal, with torch.equal, the same tracker fed the planes converted by hand -- the
tracker is bitwise reproducible from run to run (tests/test_stream_pool_gpu.py relies on the same), and the frames are the same bytes."""
import numpy as np
import pytest
import torch

import _decoder_refs as D
import _frame_refs as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = 'cuda:0'

# picture (h, w, pitch) -> output size, mode
CASES = [
    ((1, 1, 2), (1, 1), 'area'),
    ((1, 1, 2), (3, 5), 'area'),
    ((2, 2, 2), (2, 2), 'area'),
    ((7, 13, 16), (7, 13), 'area'),            # odd both ways: last row and column on the ceil chroma sample, pitch > w
    ((5, 3, 4), (11, 9), 'area'),              # enlarging, border clamp
    ((6, 10, 10), (4, 15), 'area'),            # one axis reducing, one enlarging
    ((37, 301, 304), (5, 40), 'area'),         # source footprint larger than one staged chunk on both axes
    ((9, 603, 608), (3, 130), 'area'),         # three column tiles, one of which starts on an odd source column
    ((33, 9, 10), (17, 3), 'area'),            # two row tiles, the second starts on an odd source row
    ((12, 20, 32), (7, 9), 'cubic'),
    ((12, 20, 32), (30, 50), 'cubic'),         # two row tiles, the second starts on an odd source row (asserted below)
]
TILE_H, TILE_W = 16, 64                        # FR_TH, FR_TW of csrc/frame_passes.h


def _first_source_index(mode, src, dst, d):
    """axis_span's ``first`` (csrc/frame_passes.h), clamped into the map like the kernel's R0 / C0."""
    if mode == 'area' and src >= dst:
        first = d * src // dst
    else:
        num, den = (2 * d + 1) * src - dst, 2 * dst
        fl = num // den if num >= 0 else -1
        first = fl if mode == 'area' else fl - 1
    return min(max(first, 0), src - 1)


def _adjusted(case):
    """The three-column-tile case with w moved until one tile's first source column is odd (it is at 603; the loop states the rule)."""
    (h, w, pitch), out, mode = case
    while not any(_first_source_index(mode, w, out[1], x0) % 2 for x0 in range(0, out[1], TILE_W)):
        w -= 1
    return (h, w, pitch), out, mode


def test_the_cases_reach_chunks_that_start_inside_a_chroma_pair():
    (h, w, pitch), out, mode = _adjusted(CASES[7])
    assert out[1] > 2 * TILE_W and any(_first_source_index(mode, w, out[1], x0) % 2 for x0 in range(0, out[1], TILE_W)) and pitch >= w
    for (h, w, _), out, mode in (CASES[8], CASES[10]):
        assert _first_source_index(mode, h, out[0], TILE_H) % 2 == 1, (h, out)
    (h, w, _), out, _ = CASES[6]
    assert h > 32 and w > 240 and out[0] <= TILE_H and out[1] <= TILE_W      # one tile whose footprint is 2 x 2 chunks (FR_PR, FR_PC)


def _desc(rows):
    return torch.tensor(rows, dtype=torch.int64)


def _convert_one(buf, h, w, pitch, uv_off, name, out, mode):
    from frtm_vos_amd import ops
    row = [0, h, w, ops.RESIZE_MODES[mode], ops.FRAME_FORMATS[name], pitch, uv_off, 0]
    return ops.frames_to_rgb_u8(torch.from_numpy(buf).to(DEV), _desc([row]), out)[0]


def _resize_planar(planar, out, mode):
    from frtm_vos_amd import ops
    _, h, w = planar.shape
    return ops.resize_frames_u8(torch.from_numpy(planar.reshape(-1).copy()).to(DEV), _desc([[0, h, w, ops.RESIZE_MODES[mode]]]), 3, out)[0]


@pytest.fixture(scope='module')
def case_results():
    """Every case x format once: (numpy-converted planes, fused result on the host)."""
    res = {}
    for ci, case in enumerate(CASES):
        (h, w, pitch), out, mode = _adjusted(case) if ci == 7 else case
        for fi, name in enumerate(D.NV12):
            rng = np.random.default_rng(1000 + 10 * ci + fi)
            buf, uv_off = D.random_surface(rng, h, w, pitch)
            planar = D.nv12_to_rgb(buf, 0, h, w, pitch, uv_off, name)
            got = _convert_one(buf, h, w, pitch, uv_off, name, out, mode)
            res[ci, name] = (planar, got, _resize_planar(planar, out, mode), (h, w), out, mode)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize('name', D.NV12)
@pytest.mark.parametrize('ci', range(len(CASES)), ids=['%dx%d_p%d-%dx%d-%s' % (c[0] + c[1] + (c[2],)) for c in CASES])
def test_fused_launch_is_bit_identical_to_convert_then_resize(case_results, ci, name):
    planar, got, want, size, out, mode = case_results[ci, name]
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3,) + out and got.device == torch.device(DEV)
    assert torch.equal(got, want)
    if size == out:                                                    # the resize is the identity: the numpy formula, bit for bit
        assert np.array_equal(got.cpu().numpy(), planar)
    assert int(planar.min()) == 0 and int(planar.max()) == 255 or planar.size < 100     # the clamps act


@pytest.mark.parametrize('name', D.NV12)
@pytest.mark.parametrize('ci', range(len(CASES)), ids=['%dx%d_p%d-%dx%d-%s' % (c[0] + c[1] + (c[2],)) for c in CASES])
def test_fused_launch_against_the_fp64_resize(case_results, ci, name):
    planar, got, _, size, out, mode = case_results[ci, name]
    ref = R.resize_ref(planar, out, mode)
    mism, share = R.assert_band(got.cpu().numpy(), ref, '%r %s' % (CASES[ci], name))
    print('%r %s: %d of %d outputs differ (all inside the near-tie band), band share %.4f' % (CASES[ci], name, mism, ref.size, share))
    integer_ratio = all(max(s, o) % min(s, o) == 0 for s, o in zip(size, out))
    if not integer_ratio and ref.size >= 500:
        assert share < R.BAND_CAP


# ---- one mixed launch -----------------------------------------------------------------------------------------------------------------
OUT = (6, 10)


def _mixed(seed):
    """The four rows of the mixed launch -> (buffer with zeros outside the samples, sample mask, table rows, per-row singles)."""
    from frtm_vos_amd import ops
    rng = np.random.default_rng(seed)
    planar = rng.integers(0, 256, (3, 5, 7), dtype=np.uint8)
    parts = [('rgb', planar.reshape(-1), np.ones(planar.size, dtype=bool), 5, 7, 0, 0, 'area')]
    for name, h, w, pitch, coded, mode in (('nv12_bt601', 7, 13, 16, 7, 'area'), ('nv12_bt709_full', 8, 6, 6, 8, 'area'),
                                           ('nv12_bt709', 12, 20, 32, 16, 'cubic')):
        buf, uv_off = D.random_surface(rng, h, w, pitch, coded)
        parts.append((name, buf, D.sample_mask(h, w, pitch, coded), h, w, pitch, uv_off, mode))
    gaps = (0, 7, 5, 9)                                                # 105 + 7 + 176 + 5 = 293: the third row starts at an odd byte offset
    chunks, masks, rows, off = [], [], [], 0
    for gap, (name, buf, mask, h, w, pitch, uv_off, mode) in zip(gaps, parts):
        chunks += [np.zeros(gap, dtype=np.uint8), buf]
        masks += [np.zeros(gap, dtype=bool), mask]
        off += gap
        rows.append([off, h, w, ops.RESIZE_MODES[mode], ops.FRAME_FORMATS[name], pitch, off + uv_off if name != 'rgb' else 0, 0])
        off += buf.size
    chunks.append(np.zeros(5, dtype=np.uint8))
    masks.append(np.zeros(5, dtype=bool))
    mask = np.concatenate(masks)
    buf = np.where(mask, np.concatenate(chunks), 0).astype(np.uint8)
    return buf, mask, rows, parts, planar


def test_one_mixed_launch_equals_the_single_frame_results_whatever_the_padding_holds():
    from frtm_vos_amd import ops
    buf, mask, rows, parts, planar = _mixed(5)
    assert rows[2][0] % 2 == 1 and rows[3][6] == rows[3][0] + 16 * 32 and float(mask.mean()) < 0.8
    got = ops.frames_to_rgb_u8(torch.from_numpy(buf).to(DEV), _desc(rows), OUT)
    plan = ops.FramePlan(_desc(rows), DEV)
    assert tuple(got.shape) == (4, 3) + OUT and torch.equal(plan.frames(torch.from_numpy(buf).to(DEV), OUT), got)
    assert torch.equal(got[0], _resize_planar(planar, OUT, 'area'))
    for k in (1, 2, 3):
        name, surf, _, h, w, pitch, uv_off, mode = parts[k]
        assert torch.equal(got[k], _convert_one(surf, h, w, pitch, uv_off, name, OUT, mode)), name
        assert torch.equal(got[k], _resize_planar(D.nv12_to_rgb(surf, 0, h, w, pitch, uv_off, name), OUT, mode)), name
    # every byte that is no picture sample -- row padding, rows up to the coded height, the gaps between the frames -- random instead of 0
    noise = np.random.default_rng(6).integers(0, 256, buf.size, dtype=np.uint8)
    dirty = np.where(mask, buf, noise).astype(np.uint8)
    assert int((dirty != buf).sum()) > 0.15 * buf.size
    out = torch.zeros_like(got)
    assert plan.frames(torch.from_numpy(dirty).to(DEV), OUT, out=out) is out
    assert torch.equal(out, got)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
GOOD = [0, 6, 10, 0, 3, 16, 128, 0]                                    # a 6 x 10 surface of pitch 16 and coded height 8: 176 bytes


def _row(**kw):
    keys = ['off', 'h', 'w', 'mode', 'format', 'pitch', 'uv_off']
    row = list(GOOD)
    for k, v in kw.items():
        row[keys.index(k)] = v
    return row


REFUSED = [
    (_row(h=0), 'has size 0 x 10'), (_row(w=0), 'has size 6 x 0'), (_row(h=16385), 'has size 16385 x 10'), (_row(w=16385, pitch=16386), 'has size 6 x 16385'),
    (_row(mode=2), 'has mode 2'), (_row(mode=-1), 'has mode -1'),
    (_row(format=5), 'has format 5'), (_row(format=-1), 'has format -1'),
    (_row(pitch=9), 'has pitch 9'), (_row(w=11, pitch=11), 'has pitch 11'), (_row(pitch=0), 'has pitch 0'),
    (_row(off=-1), "Y plane"), (_row(off=5000), "Y plane"), (_row(off=4096 - 95), "Y plane"), (_row(pitch=2048), "Y plane"), (_row(pitch=2 ** 62), "Y plane"),
    (_row(uv_off=-1), "chroma plane"), (_row(uv_off=4096 - 47), "chroma plane"), (_row(uv_off=5000), "chroma plane"),
    (_row(format=0, off=4096 - 179), 'leaves the 4096-byte source buffer'), (_row(format=0, off=-1), 'leaves the 4096-byte source buffer'),
]


def test_refusals_happen_on_the_host_and_leave_out_untouched():
    from frtm_vos_amd import _hip, ops
    L = _hip.lib()
    src = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 3, 6, 10), 7, dtype=torch.uint8, device=DEV)
    for row, message in REFUSED:
        plan = ops.FramePlan(_desc([row]), DEV)
        with pytest.raises(RuntimeError, match=r'frtm_frames_to_rgb_u8 failed \(-1\).*' + message):
            plan.frames(src, (6, 10), out=out)
        with pytest.raises(RuntimeError, match=message):
            ops.frames_to_rgb_u8(src, _desc([row]), (6, 10))
    # the last rows of a surface that ends exactly at the buffer's end are accepted: the bounds are tight
    edge = ops.FramePlan(_desc([_row(off=4096 - 176, uv_off=4096 - 48)]), DEV)
    scratch = torch.empty_like(out)
    edge.frames(src, (6, 10), out=scratch)
    host = _desc([GOOD])
    dev = host.to(DEV)

    def call(src_p=src.data_ptr(), host_p=host.data_ptr(), dev_p=dev.data_ptr(), n=1, out_p=out.data_ptr(), H=6, W=10):
        rc = L.frtm_frames_to_rgb_u8(src_p, src.numel(), host_p, dev_p, n, out_p, H, W, _hip.stream())
        return rc, L.frtm_last_error().decode()
    for kw in (dict(src_p=None), dict(host_p=None), dict(dev_p=None), dict(out_p=None), dict(n=0), dict(n=-3)):
        rc, msg = call(**kw)
        assert rc == -1 and 'bad argument' in msg, kw
    for kw in (dict(H=0), dict(W=0), dict(H=16385), dict(W=16385)):
        rc, msg = call(**kw)
        assert rc == -1 and 'output size' in msg, kw
    rc, msg = call(n=21846)                                           # 3 n > 65535 planes: refused before a row is read
    assert rc == -1 and 'at most 65535 planes' in msg
    torch.cuda.synchronize()
    assert int(out.min()) == 7 and int(out.max()) == 7                # nothing was launched
    assert call()[0] == 0                                             # the same call with the valid row runs
    torch.cuda.synchronize()
    assert int(out.max()) != 7 or int(out.min()) != 7
    with pytest.raises(TypeError, match='out must be'):
        ops.FramePlan(host, DEV).frames(src, (6, 10), out=out[:, :2])
    with pytest.raises(TypeError, match='flat uint8'):
        ops.FramePlan(host, DEV).frames(src.float(), (6, 10))


# ---- Tracker --------------------------------------------------------------------------------------------------------------------------
WS = (128, 160)
BIG = (256, 320)


def _params(working_size=None):
    """The configuration of tests/test_working_size_gpu.py: ResNet-18, fast parameters, a short memory."""
    from frtm_vos_amd.evaluate import Parameters
    torch.manual_seed(0)
    kw = {} if working_size is None else dict(working_size=working_size)
    params = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18', feature_batch=8, trunk_lanes=2, **kw)
    params.disc_params.update(memory_size=8, init_iters=(2, 3), update_iters=(3,))
    return params


def _nv12_sequence(name, frames, size, n_obj, seed, fmt, pitch):
    """A synthetic sequence as a decoder would deliver it -> [(DecoderFrame, the same picture converted by hand, labels, new_objects)]."""
    from frtm_vos_amd import ops
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    seq = SyntheticSequence(name, frames, size, n_obj, seed=seed)
    seq.preload(DEV)
    matrix, full = fmt.split('_')[1], fmt.endswith('_full')
    out = []
    for t, (image, labels, new_objects) in enumerate(seq):
        coded = size[0] + 8 * (t % 2)                                  # every other frame with a coded height above the picture's
        buf, uv_off = D.encode_nv12(image.cpu().numpy(), pitch, fmt, coded_h=coded, fill=(37 * t) % 256)
        by_hand = torch.from_numpy(D.nv12_to_rgb(buf, 0, size[0], size[1], pitch, uv_off, fmt)).to(DEV)
        frame = ops.DecoderFrame(torch.from_numpy(buf).to(DEV), size[0], size[1], pitch=pitch, uv_offset=uv_off, matrix=matrix, full_range=full)
        out.append((frame, by_hand, labels.to(DEV) if torch.is_tensor(labels) else labels, new_objects))
    return out


def _loop(trk, frames):
    """initialize(), then track(frame) frame by frame -> ({t: masks}, {t: native_labels or None})."""
    trk.eval()
    soft, labels = {}, {}
    for t, (image, lb, new_objects) in enumerate(frames):
        had = len(trk.targets) > 0
        if len(new_objects) > 0:
            torch.manual_seed(0)
            trk.initialize(image, lb, new_objects)
        if had:
            soft[t] = trk.track(image).clone()
            labels[t] = None if trk.native_labels is None else trk.native_labels.clone()
        trk.current_frame += 1
    torch.cuda.synchronize()
    return soft, labels


def test_tracker_on_decoder_frames_equals_the_tracker_on_frames_converted_by_hand():
    """(i) no working size: the frame is converted at its own size; every mask stack is the plain tracker's, bit for bit."""
    seq = _nv12_sequence('nv', 7, WS, 2, 61, 'nv12_bt709', 192)
    trk = _params().get_model()
    got, got_labels = _loop(trk, [(f, lb, new) for f, _, lb, new in seq])
    plans = len(trk._resize_plans)
    ref, _ = _loop(_params().get_model(), [(im, lb, new) for _, im, lb, new in seq])
    assert sorted(got) == sorted(ref) == list(range(1, 7)) and all(v is None for v in got_labels.values())
    for t in ref:
        assert tuple(got[t].shape) == (3,) + WS and torch.equal(got[t], ref[t]), t
    assert float(torch.cat([m[1:].reshape(-1) for m in ref.values()]).std()) > 1e-3      # the masks are not trivial
    assert plans == 2                                                  # one plan per surface layout (two coded heights), kept


def test_tracker_under_a_working_size_on_decoder_frames():
    """(ii) 256 x 320 surfaces at working size 128 x 160: conversion and resize in one launch; masks and native_labels bit for bit."""
    seq = _nv12_sequence('nvbig', 7, BIG, 2, 62, 'nv12_bt601', 384)
    got, got_labels = _loop(_params(WS).get_model(), [(f, lb, new) for f, _, lb, new in seq])
    trk = _params(WS).get_model()
    ref, ref_labels = _loop(trk, [(im, lb, new) for _, im, lb, new in seq])
    assert sorted(got) == sorted(ref) == list(range(1, 7)) and tuple(trk.current_masks.shape[-2:]) == WS
    for t in ref:
        assert tuple(got[t].shape) == (3,) + BIG and tuple(got_labels[t].shape) == (1,) + BIG
        assert torch.equal(got[t], ref[t]) and torch.equal(got_labels[t], ref_labels[t]), t


def test_sequence_paths_stay_tensor_only():
    """(iii)"""
    seq = _nv12_sequence('nvwin', 2, WS, 1, 63, 'nv12_bt709', 160)
    trk = _params().get_model().eval()
    torch.manual_seed(0)
    trk.initialize(seq[0][0], seq[0][2], seq[0][3])
    trk.current_frame += 1
    with pytest.raises(TypeError, match='tensor frames only'):
        trk.track_window([seq[1][0]], [None])
    with pytest.raises(TypeError, match='tensor frames only'):
        next(iter(trk.frames_with_features([(f, lb, new) for f, _, lb, new in seq])))
    assert tuple(trk.track(seq[1][0]).shape) == (2,) + WS              # the per-frame path takes it


# ---- StreamPool -----------------------------------------------------------------------------------------------------------------------
def _pool_run(streams, working_size, by_hand):
    """``streams``: per stream a list of (frame or DecoderFrame, planes converted by hand, labels, new_objects)."""
    pool = _params().get_stream_pool(max_streams=3, working_size=working_size)
    sids = [pool.open() for _ in streams]
    soft, labels = [dict() for _ in streams], [dict() for _ in streams]
    ticks = 0
    for t in range(len(streams[0])):
        frames = {}
        for k, seq in enumerate(streams):
            frame, hand, lb, new_objects = seq[t]
            image = hand if by_hand else frame
            if len(new_objects) > 0:
                torch.manual_seed(0)
                pool.initialize(sids[k], image, lb, new_objects)
            frames[sids[k]] = image
        out = pool.step(frames)
        ticks += 1 if out else 0
        for k in range(len(streams)):
            if sids[k] in out:
                soft[k][t] = out[sids[k]].clone()
                if sids[k] in pool.native_labels:
                    labels[k][t] = pool.native_labels[sids[k]].clone()
    torch.cuda.synchronize()
    counters = (pool.trunk_passes, pool.frame_launches, ticks)
    for sid in sids:
        pool.close(sid)
    return soft, labels, counters


@pytest.mark.parametrize('working_size', [None, WS], ids=['plain', 'working_size'])
def test_pool_takes_tensors_and_decoder_frames_in_one_tick(working_size):
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    third = BIG if working_size is not None else WS
    plain = SyntheticSequence('pl', 6, WS, 1, seed=70)
    plain.preload(DEV)
    streams = [[(im, im, lb, new) for im, lb, new in plain],
               _nv12_sequence('p709', 6, WS, 2, 71, 'nv12_bt709', 176),
               _nv12_sequence('p601', 6, third, 2, 72, 'nv12_bt601_full', third[1] + 32)]
    got, got_labels, (passes, launches, ticks) = _pool_run(streams, working_size, by_hand=False)
    ref, ref_labels, (ref_passes, ref_launches, ref_ticks) = _pool_run(streams, working_size, by_hand=True)
    assert ticks == ref_ticks == 5 and passes == ref_passes == 5       # one trunk pass per tick either way
    assert launches == 5 and ref_launches == 0                         # one conversion launch per tick; none for a pool fed tensors
    for k, size in enumerate((WS, WS, third)):
        assert sorted(got[k]) == sorted(ref[k]) == list(range(1, 6))
        assert sorted(got_labels[k]) == sorted(ref_labels[k]) == (list(range(1, 6)) if size != WS else [])
        for t in ref[k]:
            assert tuple(got[k][t].shape[-2:]) == size and torch.equal(got[k][t], ref[k][t]), (k, t)
        for t in ref_labels[k]:
            assert torch.equal(got_labels[k][t], ref_labels[k][t]), (k, t)
