"""The object report on the GPU: frtm_describe_frames (csrc/object_report.hip) through ops.describe_frames, Tracker.describe and
StreamPool.describe.

Every word is an exact integer function of the inputs, so every comparison is torch.equal on ALL n x 16 x 12 words against the numpy
statement of tests/_object_refs.py (which tests/test_object_report.py holds to a plain loop over pixels); there is no tolerance anywhere in
this file."""
import numpy as np
import pytest
import torch

import _object_refs as O

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = 'cuda:0'

# the tile is 16 rows x 64 columns (a wave's ballot is 64 columns of one row): single pixels, single rows and columns, one column / one row
# past a tile, several tiles both ways
SIZES = [(1, 1), (1, 64), (1, 65), (7, 13), (63, 130), (33, 257), (97, 129)]
LABEL_IDS = {1: [200], 3: [0, 3, 200], 16: [0, 3, 200, 255] + list(range(10, 22))}
FORMS = [('labels', K) for K in (1, 3, 16)] + [('masks', K) for K in (1, 2, 3, 16)]
CASES = [(size, form, K) for size in SIZES for form, K in FORMS]


def _case_input(ci):
    """-> (numpy answer, numpy ids / lut, names of the hand-placed pixels)."""
    (h, w), form, K = CASES[ci]
    rng = np.random.default_rng(300 + ci)
    if form == 'labels':
        ids = LABEL_IDS[K]
        return O.blob_labels(rng, h, w, sorted(set(ids) | {41, 0})), np.array(ids, dtype=np.uint8), []      # 41 is never listed; 0 not for K = 1
    lut = np.concatenate([[0 if ci % 2 == 0 else 7], rng.permutation(np.arange(8, 250))[:K - 1]]).astype(np.uint8)
    stack, placed = O.hand_placed(O.merged_stack(rng, K, h, w))
    return stack, lut, placed


def _describe(answers, which):
    """ops.describe_frames on numpy answers with their ids (label maps) / LUTs (stacks) -> the report."""
    from frtm_vos_amd import ops
    tensors = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in answers]
    luts = [torch.from_numpy(np.asarray(i, dtype=np.uint8)).to(DEV) if a.ndim == 3 else None for a, i in zip(answers, which)]
    ids = [None if a.ndim == 3 else [int(v) for v in i] for a, i in zip(answers, which)]
    return ops.describe_frames(tensors, luts=luts, ids=ids)


def _want(answers, which):
    return torch.from_numpy(O.report(answers, which))


@pytest.fixture(scope='module')
def matrix_results():
    out = []
    for ci in range(len(CASES)):
        answer, which, placed = _case_input(ci)
        out.append((_describe([answer], [which]).words.cpu(), _want([answer], [which]), answer, placed))
    return out


def _case_id(c):
    (h, w), form, K = c
    return '%dx%d-%s-K%d' % (h, w, form, K)


@pytest.mark.parametrize('ci', range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_report_equals_the_reference_word_for_word(matrix_results, ci):
    got, want, answer, _ = matrix_results[ci]
    (h, w), form, K = CASES[ci]
    assert got.dtype == torch.int64 and tuple(got.shape) == (1, 16, 12)
    bad = (got != want).nonzero()
    assert torch.equal(got, want), 'first differing (frame, slot, word): %r: got %r, want %r' % (bad[:8].tolist(), got[got != want][:8].tolist(),
                                                                                                 want[got != want][:8].tolist())
    assert not got[0, K:].any()
    if form == 'masks':
        assert int(want[0, :K, O.AREA].sum()) == h * w                  # every pixel of a stack has a slot
    else:
        assert int(want[0, :K, O.AREA].sum()) <= h * w and not want[0, :, O.CONF:O.MASS + 1].any()


def test_the_matrix_meets_the_hand_placed_pixels(matrix_results):
    """The stacks of the matrix hold the values the decode and q can get wrong: 0.5 exactly, a tie, a NaN next to a finite plane, NaNs only,
    a value above 1 and one below 0, a background plane larger than an object above 0.5."""
    seen = set()
    for (_, _, answer, placed), (size, form, K) in zip(matrix_results, CASES):
        if form != 'masks':
            continue
        seen |= set(placed)
        flat = answer.reshape(K, -1)
        px = {name: flat[:, flat.shape[1] - 1 - i] for i, name in enumerate(placed)}
        if 'half_is_background' in px:
            assert px['half_is_background'][1] == np.float32(0.5) and px['half_is_background'][0] == 0
        if 'tie_first_wins' in px:
            assert px['tie_first_wins'][1] == px['tie_first_wins'][2] == np.float32(0.75)
        if 'nan_next_to_finite' in px:
            assert np.isnan(px['nan_next_to_finite'][1]) and px['nan_next_to_finite'][2] == np.float32(0.625)
        if 'nans_only' in px:
            assert np.isnan(px['nans_only']).all()
        if 'above_one' in px:
            assert px['above_one'][1] > 1
        if 'below_zero' in px:
            assert px['below_zero'][1] < 0
        if 'background_above_an_object' in px:
            assert px['background_above_an_object'][0] > px['background_above_an_object'][2] > px['background_above_an_object'][1] > 0.5
    assert seen == {name for name, _, _ in O.HAND}
    full = [placed for (_, _, _, placed), (size, form, K) in zip(matrix_results, CASES) if form == 'masks' and K >= 3 and size[0] * size[1] >= 7]
    assert len(full) >= 10 and all(len(p) == len(O.HAND) for p in full)   # every larger stack of three planes and more holds all seven


# ---- geometry ---------------------------------------------------------------------------------------------------------------------------
def test_geometry():
    h, w = 21, 70
    absent = np.ones((h, w), dtype=np.uint8)                            # id 2 is measured and absent
    whole = np.full((h, w), 9, dtype=np.uint8)
    corners = np.zeros((h, w), dtype=np.uint8)
    corners[0, 0], corners[0, -1], corners[-1, 0], corners[-1, -1] = 1, 2, 3, 4
    touching = np.zeros((h, w), dtype=np.uint8)
    touching[5:12, 10:64], touching[5:12, 64:69] = 1, 2                 # they meet along the tile border, columns 63 | 64
    unlisted = np.zeros((h, w), dtype=np.uint8)
    unlisted[3:9, 3:9], unlisted[3:9, 9:12] = 5, 6                      # 6 and 0 are not listed
    stack_absent = np.zeros((3, h, w), dtype=np.float32)
    stack_absent[0], stack_absent[1, 2:4, 2:4], stack_absent[0, 2:4, 2:4] = 0.875, 0.75, 0
    stack_whole = np.stack([np.zeros((h, w), dtype=np.float32), np.full((h, w), 0.625, dtype=np.float32)])
    answers = [absent, whole, corners, touching, unlisted, stack_absent, stack_whole]
    which = [[1, 2], [9], [0, 1, 2, 3, 4], [1, 2], [5], [0, 30, 40], [0, 50]]
    rep = _describe(answers, which)
    want = _want(answers, which)
    assert torch.equal(rep.words.cpu(), want)
    W = want.numpy()
    border_all = 2 * h + 2 * w - 4
    assert W[0, 1].tolist() == [0, w, h, -1, -1, 0, 0, 0, 0, 0, 0, 2] and W[0, 0, O.AREA] == h * w                      # the sentinel box
    assert rep.objects(0)[2].box is None and rep.objects(0)[2].centroid is None and rep.objects(0)[1].box == (0, 0, w - 1, h - 1)
    assert W[1, 0].tolist() == [h * w, 0, 0, w - 1, h - 1, h * w * (w - 1) // 2, w * h * (h - 1) // 2, 0, border_all, 0, 0, 9]
    for s, (x, y) in zip((1, 2, 3, 4), ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))):
        assert W[2, s].tolist() == [1, x, y, x, y, x, y, 1, 1, 0, 0, s]                                               # a corner counts once
    assert W[2, 0, O.BORDER] == border_all - 4 and W[2, 0, O.EDGE] == 8
    # both get edge pixels along the side where they touch: every pixel of their outlines, 7 x 54 and 7 x 5 rectangles
    assert W[3, 0, O.EDGE] == 2 * 54 + 2 * 7 - 4 and W[3, 1, O.EDGE] == 2 * 5 + 2 * 7 - 4 and W[3, 0, O.XMAX] + 1 == W[3, 1, O.XMIN] == 64
    assert W[4, 0].tolist()[:5] == [36, 3, 3, 8, 8] and W[4, 0, O.EDGE] == 20 and not W[4, 1:].any()                    # the side towards 6 is an edge too
    assert W[5, 2].tolist() == [0, w, h, -1, -1, 0, 0, 0, 0, 0, 0, 40] and W[5, 1, O.AREA] == 4 and W[5, 1, O.CONF] == 4 * 191
    assert rep.objects(5)[40].soft_area == 0.0 and rep.objects(5)[30].confidence == 191 / 255.0
    assert W[6, 1].tolist() == [h * w, 0, 0, w - 1, h - 1, h * w * (w - 1) // 2, w * h * (h - 1) // 2, 0, border_all, 159 * h * w, 159 * h * w, 50]
    assert W[6, 0].tolist() == [0, w, h, -1, -1, 0, 0, 0, 0, 0, 0, 0]


# ---- one launch for frames of different sizes and forms -------------------------------------------------------------------------------
def _five():
    rng = np.random.default_rng(60)
    answers, which = [], []
    for k, (h, w, form, K) in enumerate([(9, 70, 'labels', 3), (21, 33, 'masks', 3), (5, 5, 'labels', 1), (35, 129, 'masks', 16), (18, 64, 'masks', 1)]):
        if form == 'labels':
            ids = LABEL_IDS[K]
            answers.append(O.blob_labels(rng, h, w, sorted(set(ids) | {41, 0})))
            which.append(np.array(ids, dtype=np.uint8))
        else:
            answers.append(O.hand_placed(O.merged_stack(rng, K, h, w))[0])
            which.append(rng.permutation(256)[:K].astype(np.uint8))
    return answers, which


def test_one_launch_for_five_frames_equals_five_launches():
    from frtm_vos_amd import ops
    answers, which = _five()
    tensors = [torch.from_numpy(a).to(DEV) for a in answers]
    luts = [torch.from_numpy(i).to(DEV) if a.ndim == 3 else None for a, i in zip(answers, which)]
    ids = [None if a.ndim == 3 else i.tolist() for a, i in zip(answers, which)]
    rep = ops.describe_frames(tensors, luts=luts, ids=ids)
    first = rep.words.clone()
    assert rep.K == [3, 3, 1, 16, 1] and rep.stacks == [False, True, False, True, True] and tuple(first.shape) == (5, 16, 12)
    assert torch.equal(first.cpu(), _want(answers, which))
    kept = len(ops._object_tables)
    again = ops.describe_frames(tensors, luts=luts, ids=ids)            # the same buffers again: the uploaded table is found, not made
    assert len(ops._object_tables) == kept <= ops.OBJECT_TABLES_KEPT and again.words.data_ptr() != rep.words.data_ptr()
    assert torch.equal(again.words, first)                              # integer sums: the same words whatever the order of the atomics
    for k in range(5):
        single = ops.describe_frames([tensors[k]], luts=[luts[k]], ids=[ids[k]])
        assert torch.equal(single.words[0], first[k])
        assert single.objects(0) == rep.objects(k)
    reuse = ops.describe_frames(tensors, luts=luts, ids=ids, out=again)
    assert reuse.words.data_ptr() == again.words.data_ptr() and torch.equal(reuse.words, first)


# ---- sums beyond 32 bits --------------------------------------------------------------------------------------------------------------
def test_sums_beyond_32_bits():
    from frtm_vos_amd import ops
    h, w = 2160, 3840
    labels = torch.full((h, w), 7, dtype=torch.uint8, device=DEV)
    got = ops.describe_frames([labels], ids=[[7]]).words.cpu()
    want = torch.zeros(1, 16, 12, dtype=torch.int64)
    want[0, 0] = torch.tensor([h * w, 0, 0, w - 1, h - 1, h * w * (w - 1) // 2, w * h * (h - 1) // 2, 0, 2 * h + 2 * w - 4, 0, 0, 7])
    assert h * w * (w - 1) // 2 > 2 ** 32 and torch.equal(got, want)
    del labels
    # a K = 1 stack of ones: conf = mass = 255 h w.  At 4112 x 4096 that is 2^32 - 65536: beyond a signed 32-bit sum; 16 rows more take it
    # beyond an unsigned one as well
    lut = torch.tensor([3], dtype=torch.uint8, device=DEV)
    for (h, w), bits in (((4112, 4096), 31), ((4128, 4096), 32)):
        ones = torch.full((1, h, w), 1.0, dtype=torch.float32, device=DEV)
        got = ops.describe_frames([ones], luts=[lut]).words.cpu()
        want[0, 0] = torch.tensor([h * w, 0, 0, w - 1, h - 1, h * w * (w - 1) // 2, w * h * (h - 1) // 2, 0, 2 * h + 2 * w - 4, 255 * h * w, 255 * h * w, 3])
        assert 255 * h * w > 2 ** bits and torch.equal(got, want), (h, w)
        del ones


# ---- bounds ---------------------------------------------------------------------------------------------------------------------------
CANARY = -0x5A5A5A5A5A5A5A5A


def test_a_row_that_leaves_its_buffer_raises_and_launches_nothing():
    from frtm_vos_amd import _hip as H
    answers, which = _five()
    tensors = [torch.from_numpy(a).to(DEV) for a in answers[:2]]
    id_bytes = [torch.from_numpy(i).to(DEV) for i in which[:2]]
    out = torch.full((2, 16, 12), CANARY, dtype=torch.int64, device=DEV)
    rows = [[0, 9, 70, tensors[0].data_ptr(), 9 * 70, 3, id_bytes[0].data_ptr(), 0],
            [1, 21, 33, tensors[1].data_ptr(), 4 * 3 * 21 * 33 - 1, 3, id_bytes[1].data_ptr(), 0]]      # bookkeeping that promises one byte too few
    host = torch.tensor(rows, dtype=torch.int64)
    dev = host.to(DEV)
    with pytest.raises(RuntimeError, match=r"frtm_describe_frames failed \(-1\).*frame 1's answer \(8316 bytes\) leaves its 8315-byte buffer"):
        H.call('frtm_describe_frames', host.data_ptr(), H.ptr(dev), 2, H.ptr(out), out.numel())
    with pytest.raises(RuntimeError, match=r'out holds 383 words, 2 frames need 384'):
        H.call('frtm_describe_frames', host.data_ptr(), H.ptr(dev), 2, H.ptr(out), out.numel() - 1)
    torch.cuda.synchronize()
    assert bool((out == CANARY).all())
    host[1, 4] += 1                                                     # the honest size: the same table is measured
    dev = host.to(DEV)
    H.call('frtm_describe_frames', host.data_ptr(), H.ptr(dev), 2, H.ptr(out), out.numel())
    assert torch.equal(out.cpu(), _want(answers[:2], which[:2]))


def test_a_larger_out_is_written_in_its_first_words_only():
    from frtm_vos_amd import ops
    answers, which = _five()
    tensors = [torch.from_numpy(a).to(DEV) for a in answers]
    luts = [torch.from_numpy(i).to(DEV) if a.ndim == 3 else None for a, i in zip(answers, which)]
    ids = [None if a.ndim == 3 else i.tolist() for a, i in zip(answers, which)]
    need = 5 * 16 * 12
    out = torch.full((need + 2 * 16 * 12 + 5,), CANARY, dtype=torch.int64, device=DEV)
    rep = ops.describe_frames(tensors, luts=luts, ids=ids, out=out)
    assert rep.words.data_ptr() == out.data_ptr() and tuple(rep.words.shape) == (5, 16, 12)
    assert torch.equal(out[:need].view(5, 16, 12).cpu(), _want(answers, which)) and bool((out[need:] == CANARY).all())
    two = ops.describe_frames(tensors[3:], luts=luts[3:], ids=ids[3:], out=rep)            # a report's buffer again, for fewer frames
    assert two.words.data_ptr() == out.data_ptr() and len(two) == 2 and torch.equal(two.words.cpu(), _want(answers[3:], which[3:]))
    assert torch.equal(out[2 * 16 * 12:need].view(3, 16, 12).cpu(), _want(answers[2:], which[2:])) and bool((out[need:] == CANARY).all())


# ---- Tracker and StreamPool ------------------------------------------------------------------------------------------------------------
WS = (128, 160)
BIG = (256, 320)


def _params(working_size=None):
    """The configuration of tests/test_frame_render_gpu.py: ResNet-18, fast parameters, a short memory."""
    from frtm_vos_amd.evaluate import Parameters
    torch.manual_seed(0)
    kw = {} if working_size is None else dict(working_size=working_size)
    params = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18', feature_batch=8, trunk_lanes=2, **kw)
    params.disc_params.update(memory_size=8, init_iters=(2, 3), update_iters=(3,))
    return params


def _sequence(name, frames, size, n_obj, seed):
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    seq = SyntheticSequence(name, frames, size, n_obj, seed=seed)
    seq.preload(DEV)
    return [(image, labels.to(DEV) if torch.is_tensor(labels) else labels, new_objects) for image, labels, new_objects in seq]


@pytest.mark.parametrize('working_size', [None, WS], ids=['plain', 'working_size'])
def test_tracker_describe_equals_the_reference(working_size):
    from frtm_vos_amd import ops
    size = BIG if working_size is not None else WS
    seq = _sequence('rt', 3, size, 2, 81)
    trk = _params(working_size).get_model().eval()
    with pytest.raises(ValueError, match='nothing was tracked'):
        trk.describe()
    torch.manual_seed(0)
    trk.initialize(seq[0][0], seq[0][1], seq[0][2])
    trk.current_frame += 1
    for image, _, _ in seq[1:]:
        masks = trk.track(image)
        trk.current_frame += 1
    answer = masks.cpu().numpy().copy()
    lut = trk._object_lut().cpu().numpy()
    rep = trk.describe()
    assert isinstance(rep, ops.ObjectReport) and len(rep) == 1 and rep.K == [3] and rep.stacks == [True] and tuple(answer.shape) == (3,) + size
    want = _want([answer], [lut])
    assert torch.equal(rep.words.cpu(), want)
    assert torch.equal(masks.cpu(), torch.from_numpy(answer))           # describe() reads the answer and leaves it alone
    if working_size is not None:
        assert trk.native_labels is not None and tuple(trk.native_labels.shape) == (1,) + BIG and tuple(trk.current_masks.shape[-2:]) == WS
        counts = np.bincount(trk.native_labels.cpu().numpy().reshape(-1), minlength=256)
        assert want[0, :3, O.AREA].tolist() == [int(counts[i]) for i in lut.tolist()] and int(counts.sum()) == BIG[0] * BIG[1]
    else:
        assert trk.native_labels is None and masks.data_ptr() == trk.current_masks.data_ptr()
    objs = rep.objects(0)
    print('objects of the last answer:', objs)
    assert list(objs) == lut.tolist() and sum(o.area for o in objs.values()) == size[0] * size[1]
    assert all(o.confidence is None or 0.5 < o.confidence <= 1.0 for i, o in objs.items() if i != 0) and all(o.soft_area >= 0 for o in objs.values())
    again = trk.describe(out=rep)
    assert again.words.data_ptr() == rep.words.data_ptr() and torch.equal(again.words.cpu(), want)


def test_pool_describe_is_one_launch_for_all_streams():
    streams = [_sequence('pa', 3, WS, 1, 90), _sequence('pb', 3, WS, 2, 91), _sequence('pc', 3, BIG, 2, 92), _sequence('pd', 3, (192, 224), 3, 93)]
    pool = _params().get_stream_pool(max_streams=4, working_size=WS)
    with pytest.raises(ValueError, match='nothing was tracked'):
        pool.describe()
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
    assert sorted(out) == sorted(sids) and sids[2] in pool.native_labels and sids[3] in pool.native_labels and sids[0] not in pool.native_labels
    counters = (pool.trunk_passes, pool.frame_launches, pool.refiner_passes, pool.grouped_launches, pool.render_launches)
    assert pool.describe_launches == 0
    index, rep = pool.describe()
    assert pool.describe_launches == 1 and sorted(index) == sorted(sids) and sorted(index.values()) == [0, 1, 2, 3] and len(rep) == 4
    assert (pool.trunk_passes, pool.frame_launches, pool.refiner_passes, pool.grouped_launches, pool.render_launches) == counters
    words = rep.words.cpu()
    for sid, seq, n_obj in zip(sids, streams, (1, 2, 2, 3)):
        tr = pool.tracker(sid)
        answer, lut = out[sid].cpu().numpy(), tr._object_lut().cpu().numpy()
        assert tuple(answer.shape) == (n_obj + 1,) + tuple(seq[0][0].shape[-2:]) and rep.K[index[sid]] == n_obj + 1
        want = _want([answer], [lut])[0]
        assert torch.equal(words[index[sid]], want), sid
        if sid in pool.native_labels:
            counts = np.bincount(pool.native_labels[sid].cpu().numpy().reshape(-1), minlength=256)
            assert want[:n_obj + 1, O.AREA].tolist() == [int(counts[i]) for i in lut.tolist()]
        assert sum(o.area for o in rep.objects(index[sid]).values()) == answer.shape[1] * answer.shape[2]
    some, rep2 = pool.describe([sids[3], sids[0]], out=rep)
    assert pool.describe_launches == 2 and some == {sids[3]: 0, sids[0]: 1} and rep2.words.data_ptr() == rep.words.data_ptr()
    assert torch.equal(rep2.words.cpu(), torch.stack([words[index[sids[3]]], words[index[sids[0]]]]))
    with pytest.raises(KeyError):
        pool.describe([12345])
    for sid in sids:
        pool.close(sid)
