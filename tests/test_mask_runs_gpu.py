"""The run-length coder on the GPU: frtm_encode_frames (csrc/mask_runs.hip) through ops.encode_frames, Tracker.encode and StreamPool.encode.

Every head word and every stored run length is an exact integer function of the inputs, so every comparison is an equality on ALL of them
against the numpy statement of tests/_runs_refs.py (which tests/test_mask_runs.py holds to a plain loop over pixels); there is no tolerance
anywhere in this file."""
import numpy as np
import pytest
import torch

import _runs_refs as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = 'cuda:0'
SENTINEL = -0x5A5A5A5A
CANARY = -0x5A5A5A5A5A5A5A5A

# a wave is 64 columns (lane = column) of one 64-row segment: single pixels, rows and columns, one column / one row past a tile and a segment,
# several of both, the largest sides
SIZES = [(1, 1), (1, 65), (33, 1), (2, 64), (17, 63), (33, 130), (257, 129), (1, 16384), (16384, 1),
         (63, 65), (64, 64), (65, 63), (128, 2), (129, 3)]
KS = (1, 2, 5, 16)
LABEL_IDS = [7, 0, 200, 255, 3] + list(range(10, 21))                  # slot 0 is not id 0
UNLISTED = (41, 99)
CASES = [(size, form, K) for size in SIZES for form in ('labels', 'masks') for K in KS]
CONTENTS = ['background', 'whole', 'checkerboard', 'corners', 'pair', 'pair2', 'blobs']

# stack values the decode can get wrong: {plane: value} of one pixel (the other planes 0), None: every plane a NaN; the K it needs
HAND = [(2, {1: 0.5}), (3, {1: 0.75, 2: 0.75}), (3, {1: np.nan, 2: 0.625}), (1, None), (2, {1: 1.5}), (2, {1: -0.25}), (3, {0: 0.9, 1: 0.75, 2: 0.8})]


def _planes(content, h, w, K, rng, labels):
    """(h, w) int64 in -1 .. K - 1: the slot every pixel shall have (-1: none; label maps only)."""
    p = np.zeros((h, w), dtype=np.int64)
    top = K - 1
    if content == 'whole':
        p[:] = top                                                      # the first count of slot `top` is 0
    elif content == 'checkerboard':
        p = np.add.outer(np.arange(h), np.arange(w)) % 2 * (top if top else -1)      # every pixel a boundary: the most runs
    elif content == 'corners':
        for k, (y, x) in enumerate(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1))):
            p[y, x] = min(k + 1, top) if top else -1
    elif content in ('pair', 'pair2') and w >= 2:
        x = min(63, w - 2)                                              # across a tile border when there is one
        p[h - 1, x] = top if top else -1                                # one run from the bottom of a column into the top of the next
        p[0, x + 1] = (max(top - 1, 0) if content == 'pair2' else top) if top else -1
    elif content == 'blobs':
        p = R.blob_labels(rng, h, w, list(range(K + 1 if labels else K))).astype(np.int64) - (1 if labels else 0)      # label maps: with pixels of no slot
    return p


def _frame(content, h, w, form, K, rng):
    """-> (numpy answer, ids / LUT)."""
    p = _planes(content, h, w, K, rng, form == 'labels')
    if form == 'labels':
        ids = np.array(LABEL_IDS[:K], dtype=np.uint8)
        labels = np.where(p >= 0, ids[np.maximum(p, 0)], UNLISTED[0]).astype(np.uint8)
        if content == 'blobs':
            labels[(rng.random((h, w)) < 0.1) & (p < 0)] = UNLISTED[1]    # two unlisted ids side by side: no boundary of any slot
        return labels, ids
    lut = np.concatenate([[7 if content == 'blobs' else 0], rng.permutation(np.arange(8, 250))[:K - 1]]).astype(np.uint8)
    stack = R.stack_of(np.maximum(p, 0), K, rng)
    if content == 'blobs':
        flat, placed = stack.reshape(K, -1), 0
        for planes, case in HAND:                                       # over the last pixels of the picture
            if planes <= K and placed < h * w:
                i = h * w - 1 - placed
                flat[:, i] = np.nan if case is None else 0
                for k, v in (case or {}).items():
                    flat[k, i] = v
                placed += 1
    return stack, lut


def _case_frames(ci):
    (h, w), form, K = CASES[ci]
    rng = np.random.default_rng(500 + ci)
    frames = [_frame(c, h, w, form, K, rng) for c in CONTENTS]
    return [a for a, _ in frames], [i for _, i in frames]


def _tensors(answers, which):
    tensors = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in answers]
    luts = [torch.from_numpy(np.asarray(i, dtype=np.uint8)).to(DEV) if a.ndim == 3 else None for a, i in zip(answers, which)]
    ids = [None if a.ndim == 3 else [int(v) for v in i] for a, i in zip(answers, which)]
    return tensors, luts, ids


def _encode(answers, which, capacity, pad=16, given=None):
    """ops.encode_frames into buffers of our own: heads full of CANARY, runs of capacity + pad SENTINELs -> (MaskRuns, the whole runs buffer)."""
    from frtm_vos_amd import ops
    tensors, luts, ids = given if given is not None else _tensors(answers, which)
    n = len(answers)
    buf = torch.full((capacity + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    heads = torch.full((n, 16, 4), CANARY, dtype=torch.int64, device=DEV)
    out = ops.MaskRuns(heads, buf, [a.shape[-2:] for a in answers], [len(i) for i in which], capacity + pad)
    coded = ops.encode_frames(tensors, luts=luts, ids=ids, out=out, capacity=capacity)
    assert coded.runs.data_ptr() == buf.data_ptr() and coded.heads.data_ptr() == heads.data_ptr() and coded.capacity == capacity
    return coded, buf


def _assert_equal(coded, buf, want_heads, want_runs, needed, capacity, what=''):
    heads = coded.heads.cpu()
    bad = (heads != torch.from_numpy(want_heads)).nonzero()
    assert bad.numel() == 0, '%s first differing (frame, slot, word): %r: got %r, want %r' % (
        what, bad[:6].tolist(), [int(heads[tuple(b)]) for b in bad[:6]], [int(want_heads[tuple(b)]) for b in bad[:6].tolist()])
    host = buf.cpu().numpy().astype(np.int64)
    stored = min(needed, capacity)
    diff = np.flatnonzero(host[:stored] != want_runs[:stored])
    assert diff.size == 0, '%s first differing run elements %r: got %r, want %r' % (what, diff[:8].tolist(), host[diff[:8]].tolist(), want_runs[diff[:8]].tolist())
    assert (host[stored:] == SENTINEL).all(), '%s elements at %r beyond min(needed, capacity) = %d were written' % (
        what, (stored + np.flatnonzero(host[stored:] != SENTINEL)[:8]).tolist(), stored)


@pytest.fixture(scope='module')
def matrix_results():
    out = []
    for ci in range(len(CASES)):
        answers, which = _case_frames(ci)
        want_heads, want_runs, needed = R.layout(answers, which)
        coded, buf = _encode(answers, which, needed)
        out.append((coded.heads.cpu(), buf.cpu(), want_heads, want_runs, needed, coded, answers, which))
    return out


def _case_id(c):
    (h, w), form, K = c
    return '%dx%d-%s-K%d' % (h, w, form, K)


@pytest.mark.parametrize('ci', range(len(CASES)), ids=[_case_id(c) for c in CASES])
def test_heads_and_runs_equal_the_reference_element_for_element(matrix_results, ci):
    """Seven frames per case -- all background, one object everywhere, a checkerboard, the four corners, a run across a column end with one
    object and with two, random blobs (label maps: with unlisted ids; stacks: with NaN planes, ties and 0.5) -- coded by ONE call."""
    heads, buf, want_heads, want_runs, needed, coded, answers, which = matrix_results[ci]
    (h, w), form, K = CASES[ci]
    assert heads.dtype == torch.int64 and tuple(heads.shape) == (len(CONTENTS), 16, 4) and buf.dtype == torch.int32
    _assert_equal(coded, buf, want_heads, want_runs, needed, needed, _case_id(CASES[ci]))
    assert not heads[:, K:].any()
    N = h * w
    # what the frames were built to show, read from the REFERENCE: [N], [0, N], the most runs, the run across a column end
    first = lambda f, s: want_runs[want_heads[f, s, R.OFFSET]:want_heads[f, s, R.OFFSET] + want_heads[f, s, R.COUNT]].tolist()
    assert first(0, 0) == [0, N] and all(first(0, s) == [N] for s in range(1, K))                 # slot 0 everywhere
    assert first(1, K - 1) == [0, N]
    if K > 1:
        assert want_heads[2, 0, R.COUNT] in (N + 1, N + 1 - (w - 1) * (1 - h % 2)) and want_heads[2, 0, R.COUNT] > N // 2
    if w >= 2 and K > 1:
        x = min(63, w - 2)
        p = x * h + h - 1                                                # (h - 1, x), and (0, x + 1) right behind it
        assert first(4, K - 1) == [p, 2] + ([N - p - 2] if N - p - 2 else [])
    if form == 'masks':
        assert int(want_heads[:, :K, R.AREA].sum()) == len(CONTENTS) * N                          # every pixel of a stack has a slot
    # the copy a caller makes: every slot's list decodes to the slot's mask
    from frtm_vos_amd import ops
    for f in (3, 6):
        slot = R.slots(answers[f], which[f])
        got = coded.rle(f)
        assert list(got) == [int(v) for v in which[f]]
        for s, oid in enumerate(int(v) for v in which[f]):
            assert got[oid]['size'] == [h, w] and np.array_equal(ops.rle_decode((h, w), got[oid]['counts']), slot == s), (f, s)


def test_the_matrix_meets_the_hand_placed_pixels(matrix_results):
    seen = 0
    for (_, _, _, _, _, _, answers, _), ((h, w), form, K) in zip(matrix_results, CASES):
        if form == 'masks' and K >= 3 and h * w >= len(HAND):
            flat = answers[6].reshape(K, -1)
            assert flat[1, -1] == np.float32(0.5) and flat[1, -2] == flat[2, -2] == np.float32(0.75) and np.isnan(flat[1, -3]) and np.isnan(flat[:, -4]).all()
            assert R.slots(answers[6], np.zeros(K))[np.unravel_index([h * w - 1, h * w - 2, h * w - 3, h * w - 4, h * w - 7], (h, w))].tolist() == [0, 1, 2, 0, 0]
            seen += 1
    assert seen >= 20


# ---- five mixed frames ------------------------------------------------------------------------------------------------------------------
def _five():
    rng = np.random.default_rng(61)
    answers, which = [], []
    for k, (h, w, form, K) in enumerate([(9, 70, 'labels', 3), (70, 33, 'masks', 3), (5, 5, 'labels', 1), (35, 129, 'masks', 16), (130, 64, 'masks', 1)]):
        a, i = _frame('blobs', h, w, form, K, rng)
        answers.append(a)
        which.append(i)
    return answers, which


def test_one_call_for_five_mixed_frames_equals_five_calls_with_the_offsets_shifted():
    from frtm_vos_amd import ops
    answers, which = _five()
    tensors, luts, ids = _tensors(answers, which)
    want_heads, want_runs, needed = R.layout(answers, which)
    coded = ops.encode_frames(tensors, luts=luts, ids=ids)
    assert coded.K == [3, 3, 1, 16, 1] and coded.sizes == [(9, 70), (70, 33), (5, 5), (35, 129), (130, 64)]
    assert coded.capacity == ops.default_run_capacity(coded.sizes, coded.K) == coded.runs.numel() >= needed and coded.runs.dtype == torch.int32
    heads, runs = coded.cpu()
    assert torch.equal(heads, torch.from_numpy(want_heads)) and runs.numel() == needed and np.array_equal(runs.numpy(), want_runs)
    # area = word 0 of describe_frames, on the same table (the two calls share the uploaded one)
    kept = len(ops._object_tables)
    report = ops.describe_frames(tensors, luts=luts, ids=ids)
    assert len(ops._object_tables) == kept
    assert torch.equal(report.words[:, :, 0].cpu(), heads[:, :, R.AREA]) and torch.equal(report.words[:, :, 11].cpu(), heads[:, :, R.ID])
    shift = 0
    for k in range(5):
        single = ops.encode_frames([tensors[k]], luts=[luts[k]], ids=[ids[k]])
        h1, r1 = single.cpu()
        moved = heads[k].clone()
        moved[:coded.K[k], R.OFFSET] -= shift
        assert torch.equal(h1[0], moved) and int(h1[0, 0, R.OFFSET]) == 0
        assert torch.equal(r1, runs[shift:shift + r1.numel()]) and single.counts(0) == coded.counts(k)
        shift += r1.numel()
    assert shift == needed
    for k in range(5):
        slot = R.slots(answers[k], which[k])
        for s, (oid, r) in enumerate(coded.rle(k, compressed=True).items()):
            assert oid == int(which[k][s]) and np.array_equal(ops.rle_decode(r['size'], r['counts']), slot == s)


def test_two_calls_give_identical_bytes():
    answers, which = _five()
    given = _tensors(answers, which)
    _, _, needed = R.layout(answers, which)
    a, buf_a = _encode(answers, which, needed, given=given)
    b, buf_b = _encode(answers, which, needed, given=given)
    assert buf_a.data_ptr() != buf_b.data_ptr() and torch.equal(buf_a, buf_b) and torch.equal(a.heads, b.heads)


# ---- capacity ---------------------------------------------------------------------------------------------------------------------------
def test_capacity_cuts_the_concatenation_and_nothing_else():
    from frtm_vos_amd import ops
    answers, which = _five()
    given = _tensors(answers, which)
    want_heads, want_runs, needed = R.layout(answers, which)
    for capacity in (needed, needed - 1, needed // 2, 1):
        coded, buf = _encode(answers, which, capacity, given=given)
        _assert_equal(coded, buf, want_heads, want_runs, needed, capacity, 'capacity %d' % capacity)      # the heads hold the truth, overflow or not
        if capacity == needed:
            assert np.array_equal(coded.cpu()[1].numpy(), want_runs)
        else:
            with pytest.raises(ops.RunsOverflow, match='capacity=%d' % needed) as e:
                coded.cpu()
            assert (e.value.needed, e.value.capacity) == (needed, capacity)
    # what the message says to do
    again = ops.encode_frames(given[0], luts=given[1], ids=given[2], capacity=e.value.needed)
    assert np.array_equal(again.cpu()[1].numpy(), want_runs)


def test_a_larger_out_is_written_in_its_first_elements_only():
    from frtm_vos_amd import ops
    answers, which = _five()
    tensors, luts, ids = _tensors(answers, which)
    want_heads, want_runs, needed = R.layout(answers, which)
    heads = torch.full((8, 16, 4), CANARY, dtype=torch.int64, device=DEV)
    runs = torch.full((needed + 1000,), SENTINEL, dtype=torch.int32, device=DEV)
    out = ops.MaskRuns(heads, runs, [(1, 1)] * 8, [1] * 8, runs.numel())
    coded = ops.encode_frames(tensors, luts=luts, ids=ids, out=out)         # capacity: all that out holds
    assert coded.capacity == needed + 1000 and coded.heads.data_ptr() == heads.data_ptr() and tuple(coded.heads.shape) == (5, 16, 4)
    assert torch.equal(heads[:5].cpu(), torch.from_numpy(want_heads)) and bool((heads[5:] == CANARY).all())
    assert np.array_equal(runs[:needed].cpu().numpy(), want_runs) and bool((runs[needed:] == SENTINEL).all())
    two = ops.encode_frames(tensors[3:], luts=luts[3:], ids=ids[3:], out=coded)            # the buffers again, for fewer frames
    h2, r2, n2 = R.layout(answers[3:], which[3:])
    assert two.heads.data_ptr() == heads.data_ptr() and len(two) == 2 and torch.equal(two.heads.cpu(), torch.from_numpy(h2))
    assert np.array_equal(two.cpu()[1].numpy(), r2) and np.array_equal(runs[n2:needed].cpu().numpy(), want_runs[n2:]) and bool((runs[needed:] == SENTINEL).all())


def test_a_row_that_leaves_its_buffer_raises_and_launches_nothing():
    from frtm_vos_amd import _hip as H
    answers, which = _five()
    tensors = [torch.from_numpy(a).to(DEV) for a in answers[:2]]
    id_bytes = [torch.from_numpy(i).to(DEV) for i in which[:2]]
    heads = torch.full((2, 16, 4), CANARY, dtype=torch.int64, device=DEV)
    runs = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
    rows = [[0, 9, 70, tensors[0].data_ptr(), 9 * 70, 3, id_bytes[0].data_ptr(), 0],
            [1, 70, 33, tensors[1].data_ptr(), 4 * 3 * 70 * 33 - 1, 3, id_bytes[1].data_ptr(), 0]]      # bookkeeping that promises one byte too few
    host = torch.tensor(rows, dtype=torch.int64)
    dev = host.to(DEV)
    L = H.lib()
    assert L.frtm_encode_work_bytes(host.data_ptr(), 2, 4096) == 0 and "frame 1's answer (27720 bytes) leaves its 27719-byte buffer" in L.frtm_last_error().decode()
    work = torch.full((1 << 16,), CANARY, dtype=torch.int64, device=DEV)
    args = lambda: (host.data_ptr(), H.ptr(dev), 2, H.ptr(heads), heads.numel(), H.ptr(runs), runs.numel(), H.ptr(work), work.numel() * 8)
    with pytest.raises(RuntimeError, match=r"frtm_encode_frames failed \(-1\).*frame 1's answer \(27720 bytes\) leaves its 27719-byte buffer"):
        H.call('frtm_encode_frames', *args())
    host[1, 4] += 1                                                     # the honest size
    dev = host.to(DEV)
    need = L.frtm_encode_work_bytes(host.data_ptr(), 2, 4096)
    assert 0 < need <= work.numel() * 8
    with pytest.raises(RuntimeError, match=r'work holds %d bytes, frtm_encode_work_bytes asks for %d' % (need - 8, need)):
        H.call('frtm_encode_frames', *(args()[:8] + (need - 8,)))
    with pytest.raises(RuntimeError, match=r'heads holds 127 words, 2 frames need 128'):
        H.call('frtm_encode_frames', *(args()[:4] + (127,) + args()[5:]))
    torch.cuda.synchronize()
    assert bool((heads == CANARY).all()) and bool((runs == SENTINEL).all()) and bool((work == CANARY).all())
    H.call('frtm_encode_frames', *args())                               # the same table is coded
    want_heads, want_runs, needed = R.layout(answers[:2], which[:2])
    assert torch.equal(heads.cpu(), torch.from_numpy(want_heads)) and np.array_equal(runs[:needed].cpu().numpy(), want_runs)
    assert bool((runs[needed:] == SENTINEL).all()) and bool((work.view(-1)[(need + 7) // 8:] == CANARY).all())


# ---- Tracker and StreamPool ------------------------------------------------------------------------------------------------------------
WS = (128, 160)
BIG = (256, 320)


def _params(working_size=None):
    """The configuration of tests/test_object_report_gpu.py: ResNet-18, fast parameters, a short memory."""
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
def test_tracker_encode_equals_the_reference(working_size):
    from frtm_vos_amd import ops
    size = BIG if working_size is not None else WS
    seq = _sequence('rt', 3, size, 2, 81)
    trk = _params(working_size).get_model().eval()
    with pytest.raises(ValueError, match='nothing was tracked'):
        trk.encode()
    torch.manual_seed(0)
    trk.initialize(seq[0][0], seq[0][1], seq[0][2])
    trk.current_frame += 1
    for image, _, _ in seq[1:]:
        masks = trk.track(image)
        trk.current_frame += 1
    answer = masks.cpu().numpy().copy()
    lut = trk._object_lut().cpu().numpy()
    coded = trk.encode()
    assert isinstance(coded, ops.MaskRuns) and len(coded) == 1 and coded.K == [3] and coded.sizes == [size] and tuple(answer.shape) == (3,) + size
    want_heads, want_runs, needed = R.layout([answer], [lut])
    heads, runs = coded.cpu()                                            # the default capacity holds a real answer
    print('tracker answer %r: %d run lengths of a default capacity of %d' % (size, needed, coded.capacity))
    assert torch.equal(heads, torch.from_numpy(want_heads)) and np.array_equal(runs.numpy(), want_runs)
    assert torch.equal(masks.cpu(), torch.from_numpy(answer))           # encode() reads the answer and leaves it alone
    assert torch.equal(trk.describe().words[0, :, 0].cpu(), heads[0, :, R.AREA])
    slot = R.slots(answer, lut)
    for s, (oid, r) in enumerate(coded.rle(0).items()):
        assert oid == int(lut[s]) and np.array_equal(ops.rle_decode(r['size'], r['counts']), slot == s)
    if working_size is not None:
        assert trk.native_labels is not None and tuple(trk.native_labels.shape) == (1,) + BIG and tuple(trk.current_masks.shape[-2:]) == WS
        labels = trk.native_labels.cpu().numpy()[0]
        for oid, r in coded.rle(0).items():
            assert np.array_equal(ops.rle_decode(r['size'], r['counts']), labels == oid)
    again = trk.encode(out=coded)
    assert again.runs.data_ptr() == coded.runs.data_ptr() and np.array_equal(again.cpu()[1].numpy(), want_runs)
    short = trk.encode(capacity=needed - 1)
    with pytest.raises(ops.RunsOverflow) as e:
        short.cpu()
    assert e.value.needed == needed and torch.equal(short.heads.cpu(), heads)


def test_pool_encode_is_one_call_for_all_streams():
    streams = [_sequence('pa', 3, WS, 1, 90), _sequence('pb', 3, WS, 2, 91), _sequence('pc', 3, BIG, 2, 92), _sequence('pd', 3, (192, 224), 3, 93)]
    pool = _params().get_stream_pool(max_streams=4, working_size=WS)
    with pytest.raises(ValueError, match='StreamPool.encode: no stream has an answer'):
        pool.encode()
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
    counters = lambda: (pool.trunk_passes, pool.frame_launches, pool.refiner_passes, pool.grouped_launches, pool.render_launches, pool.describe_launches)
    before = counters()
    assert pool.encode_launches == 0
    index, coded = pool.encode()
    assert pool.encode_launches == 1 and sorted(index) == sorted(sids) and sorted(index.values()) == [0, 1, 2, 3] and len(coded) == 4
    assert counters() == before
    order = sorted(sids, key=lambda sid: index[sid])
    answers = [out[sid].cpu().numpy() for sid in order]
    luts = [pool.tracker(sid)._object_lut().cpu().numpy() for sid in order]
    assert coded.K == [a.shape[0] for a in answers] and sorted(coded.K) == [2, 3, 3, 4] and len(set(coded.sizes)) == 3
    want_heads, want_runs, needed = R.layout(answers, luts)
    heads, runs = coded.cpu()
    print('pool answers: %d run lengths of a default capacity of %d' % (needed, coded.capacity))
    assert torch.equal(heads, torch.from_numpy(want_heads)) and np.array_equal(runs.numpy(), want_runs)
    for sid in sids:
        if sid in pool.native_labels:
            labels = pool.native_labels[sid].cpu().numpy()
            for oid, r in coded.rle(index[sid]).items():
                assert np.array_equal(R.decode_counts(tuple(r['size']), r['counts']), labels == oid)
    some, coded2 = pool.encode([sids[3], sids[0]], out=coded)
    assert pool.encode_launches == 2 and some == {sids[3]: 0, sids[0]: 1} and coded2.runs.data_ptr() == coded.runs.data_ptr()
    assert coded2.counts(0) == coded.counts(index[sids[3]]) and coded2.counts(1) == coded.counts(index[sids[0]])
    assert counters() == before
    with pytest.raises(KeyError):
        pool.encode([12345])
    for sid in sids:
        pool.close(sid)
