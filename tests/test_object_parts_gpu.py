"""The cleaning of an answer on the GPU (csrc/object_parts.hip, ops.clean_frames, Tracker.clean, StreamPool.clean) against the numpy
statement of tests/_parts_refs.py: every word, every byte of every cleaned map and every name of every component map compared with ``==``.
There is no tolerance in this file.  Canaries sit behind every output, and the status word of every frame is asserted to be 0."""
import numpy as np
import pytest
import torch

import _object_refs as O
import _parts_refs as P
import _runs_refs as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]
DEV = 'cuda:0'
BYTE = 0x5A                                                              # canary of a label byte
NAME = -0x5A5A5A5A                                                       # of a component name
WORD = -0x5A5A5A5A5A5A5A5A                                               # of a 64-bit word


def _tile():
    from frtm_vos_amd import ops
    return ops.PARTS_TILE_H, ops.PARTS_TILE_W


def _sizes():
    th, tw = _tile()
    return [(1, 1), (1, 65), (33, 1), (2, 64), (17, 63), (63, 65), (64, 64), (65, 63), (33, 130), (257, 129), (128, 2), (129, 3), (1, 16384), (16384, 1),
            (th - 1, tw - 1), (th, tw), (th + 1, tw + 1), (th - 1, tw + 1), (th + 1, tw - 1)]      # one below, at and one above each tile side


KS = (1, 2, 5, 16)
IDS = [0, 7, 200, 255, 3] + list(range(10, 21))                         # slot 1 holds 7: the rule with fill = 7 leaves it alone and rules slot 0
UNLISTED = (41, 99)
CONTENTS = P.PICTURES + ('blobs', 'blobs_noise')
RULES = [dict(min_area=1, largest_only=False, fill=0), dict(min_area=5, largest_only=False, fill=0), dict(min_area=1, largest_only=True, fill=0),
         dict(min_area=5, largest_only=True, fill=7)]
CALLS = [dict(rule, connectivity=c) for c in (4, 8) for rule in RULES]

# stack values the decode can get wrong: {plane: value} of one pixel (the other planes 0), None: every plane a NaN; the K it needs
HAND = [(2, {1: 0.5}), (3, {1: 0.75, 2: 0.75}), (3, {1: np.nan, 2: 0.625}), (1, None), (2, {1: 1.5}), (2, {1: -0.25}), (3, {0: 0.9, 1: 0.75, 2: 0.8})]


def _planes(content, h, w, K, rng, labels):
    """(h, w) int64 in -1 .. K - 1: the slot every pixel shall have (-1: none; label maps only)."""
    top = K - 1
    if content in ('blobs', 'blobs_noise'):
        p = R.blob_labels(rng, h, w, list(range(K + 1 if labels else K))).astype(np.int64) - (1 if labels else 0)      # label maps: with pixels of no slot
        if content == 'blobs_noise':
            p[rng.random((h, w)) < 0.5] = top                           # uniform noise in one slot: many parts, long chains of equivalences
        return p
    p = P.picture(content, h, w, o=max(top, 1), o2=max(top - 1, 1), tile=_tile(), rng=rng)
    if top == 0:
        p = np.where(p > 0, 0, -1) if labels else np.zeros_like(p)       # one slot: the object in slot 0 on pixels of no slot; a stack has only slot 0
    return p


def _frame(content, h, w, form, K, rng):
    """-> (numpy answer, ids / LUT)."""
    p = _planes(content, h, w, K, rng, form == 'labels')
    ids = np.array(IDS[:K], dtype=np.uint8)
    if form == 'labels':
        labels = np.where(p >= 0, ids[np.maximum(p, 0)], UNLISTED[0]).astype(np.uint8)
        if content.startswith('blobs'):
            labels[(rng.random((h, w)) < 0.1) & (p < 0)] = UNLISTED[1]    # two unlisted ids: both keep their byte
        return labels, ids
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
    return stack, ids


def _matrix_frames():
    """Every size x form x K x content, and one (480, 854) frame -> (descriptions, answers, ids)."""
    what, answers, which = [], [], []
    for si, (h, w) in enumerate(_sizes()):
        for form in ('labels', 'masks'):
            for K in KS:
                rng = np.random.default_rng(700 + 16 * si + K)
                for content in CONTENTS:
                    a, i = _frame(content, h, w, form, K, rng)
                    what.append('%dx%d %s K=%d %s' % (h, w, form, K, content))
                    answers.append(a)
                    which.append(i)
    a, i = _frame('blobs_noise', 480, 854, 'labels', 5, np.random.default_rng(699))
    return what + ['480x854 labels K=5 blobs_noise'], answers + [a], which + [i]


def _tensors(answers, which):
    tensors = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in answers]
    luts = [torch.from_numpy(np.asarray(i, dtype=np.uint8)).to(DEV) if a.ndim == 3 else None for a, i in zip(answers, which)]
    ids = [None if a.ndim == 3 else [int(v) for v in i] for a, i in zip(answers, which)]
    return tensors, luts, ids


def _clean(answers, which, given=None, components=True, pad=48, **rule):
    """ops.clean_frames into buffers of our own, full of canaries and ``pad`` elements longer than needed -> the CleanedAnswers."""
    from frtm_vos_amd import ops
    tensors, luts, ids = given if given is not None else _tensors(answers, which)
    n = len(answers)
    sizes = [a.shape[-2:] for a in answers]
    pixels = sum((h * w + 15) // 16 * 16 for h, w in sizes)
    label_buf = torch.full((pixels + pad,), BYTE, dtype=torch.uint8, device=DEV)
    comp_buf = torch.full((pixels + pad,), NAME, dtype=torch.int32, device=DEV)
    word_buf = torch.full((n * 193 + pad,), WORD, dtype=torch.int64, device=DEV)
    out = ops.CleanedAnswers(label_buf, comp_buf, word_buf, sizes, [len(i) for i in which], [None] * n)
    c = ops.clean_frames(tensors, luts=luts, ids=ids, components=components, out=out, **rule)
    assert c.label_buf.data_ptr() == label_buf.data_ptr() and c.word_buf.data_ptr() == word_buf.data_ptr() and len(c) == n
    assert (c.comp_buf is None) == (not components) and c.sizes == [tuple(s) for s in sizes]
    c.test_buffers = (label_buf, comp_buf, word_buf)
    return c


def _assert_equal(c, answers, which, names, what, components=True, **rule):
    """Every output of ``c`` against the reference, and every canary.  ``names``: the reference's part names per frame (they depend on the
    connectivity only)."""
    label_buf, comp_buf, word_buf = (t.cpu().numpy() for t in c.test_buffers)
    n = len(answers)
    words, status = word_buf[:192 * n].reshape(n, 16, 12), word_buf[192 * n:193 * n]
    assert (status == 0).all(), 'status of frames %r: %r' % (np.flatnonzero(status)[:8].tolist(), status[np.flatnonzero(status)[:8]].tolist())
    assert (word_buf[193 * n:] == WORD).all(), 'words beyond the n x 193 were written'
    used = np.zeros(label_buf.size, dtype=bool)
    for i, (a, ids) in enumerate(zip(answers, which)):
        h, w = a.shape[-2:]
        o = c.offsets[i]
        used[o:o + h * w] = True
        want_labels, want_comp, want_words = P.clean(a, ids, part_names=names[i], **rule)
        bad = np.argwhere(words[i] != want_words)
        assert bad.size == 0, '%s: first differing (slot, word) %r: got %r, want %r' % (
            what[i], bad[:6].tolist(), [int(words[i][tuple(b)]) for b in bad[:6]], [int(want_words[tuple(b)]) for b in bad[:6]])
        got = label_buf[o:o + h * w].reshape(h, w)
        bad = np.argwhere(got != want_labels)
        assert bad.size == 0, '%s: %d differing label bytes, first (y, x) %r: got %r, want %r' % (
            what[i], len(bad), bad[:6].tolist(), [int(got[tuple(b)]) for b in bad[:6]], [int(want_labels[tuple(b)]) for b in bad[:6]])
        if components:
            got = comp_buf[o:o + h * w].reshape(h, w)
            bad = np.argwhere(got != want_comp)
            assert bad.size == 0, '%s: %d differing names, first (y, x) %r: got %r, want %r' % (
                what[i], len(bad), bad[:6].tolist(), [int(got[tuple(b)]) for b in bad[:6]], [int(want_comp[tuple(b)]) for b in bad[:6]])
    assert (label_buf[~used] == BYTE).all(), 'label bytes between or behind the frames were written'
    assert (comp_buf[~used] == NAME).all() if components else (comp_buf == NAME).all(), 'component names outside the frames were written'


@pytest.fixture(scope='module')
def matrix():
    what, answers, which = _matrix_frames()
    slots = [P.slots(a, i) for a, i in zip(answers, which)]
    names = {c: [P.names(s, c) for s in slots] for c in (4, 8)}
    return what, answers, which, _tensors(answers, which), names, slots


def _call_id(kw):
    return 'conn%d-min%d-%s-fill%d' % (kw['connectivity'], kw['min_area'], 'largest' if kw['largest_only'] else 'all', kw['fill'])


@pytest.mark.parametrize('kw', CALLS, ids=[_call_id(kw) for kw in CALLS])
def test_words_labels_and_names_equal_the_reference(matrix, kw):
    """The whole matrix -- every size x form x K x content, and the (480, 854) frame -- in ONE call per connectivity and rule."""
    what, answers, which, given, names, slots = matrix
    assert len(answers) == len(_sizes()) * 2 * len(KS) * len(CONTENTS) + 1 <= 65535
    c = _clean(answers, which, given=given, **kw)
    _assert_equal(c, answers, which, names[kw['connectivity']], what, **kw)
    if kw['min_area'] == 1 and not kw['largest_only']:                  # the identity on slots: the cleaned map is the decoded input
        for i, (a, ids, s) in enumerate(zip(answers, which, slots)):
            decoded = a if a.ndim == 2 else np.asarray(ids, dtype=np.uint8)[s]
            assert np.array_equal(c.labels[i].cpu().numpy(), decoded), what[i]
            if i % 97 == 0:
                assert (c.cpu()[0][i, :len(ids), P.KEPT] == c.cpu()[0][i, :len(ids), P.PARTS]).all()


def test_the_matrix_meets_the_pictures_and_the_hand_placed_pixels(matrix):
    what, answers, which, _, names, slots = matrix
    th, tw = _tile()
    find = lambda text: what.index(text)
    count = lambda i, conn, s: len(np.unique(names[conn][i][slots[i] == s]))
    i = find('%dx%d masks K=2 checker' % (th + 1, tw + 1))
    assert count(i, 4, 1) == ((th + 1) * (tw + 1)) // 2 and count(i, 8, 1) == 1 and count(i, 8, 0) == 1      # two parts spanning every tile
    i = find('63x65 labels K=5 diagonal')
    assert count(i, 8, 4) == 1 and count(i, 4, 4) == 63
    for content in ('spiral', 'comb', 'comb_mirrored', 'serpentine'):
        i = find('257x129 masks K=16 ' + content)
        assert count(i, 4, 15) == 1 and (slots[i] == 15).sum() > 257 * 129 // 2 - 400, content      # one part crossing every seam
    i = find('257x129 labels K=5 ring')
    assert count(i, 4, 4) == 1 and count(i, 4, 3) == 1 and count(i, 4, 0) == 2        # the background inside the ring: an enclosed part of the unruled slot
    i = find('64x64 masks K=2 equal')
    assert count(i, 8, 1) == 2 and (np.bincount(names[8][i][slots[i] == 1])[[0, 64 * 64 - 2 - 2 * 64]] == 6).all()
    i = find('63x65 labels K=5 corners')
    assert count(i, 4, 4) == 6 and count(i, 8, 4) == 5 and count(i, 8, 3) == 1 and count(i, 4, 3) == 2        # both sides of the seam corner
    i = find('480x854 labels K=5 blobs_noise')
    assert count(i, 4, 4) > 10000 and (slots[i] < 0).any()
    i = find('33x130 masks K=5 blobs')
    s = slots[i].reshape(-1)
    assert s[-7:].tolist() == [0, 0, 1, 0, 2, 1, 0]                      # HAND, the last placed first: background plane largest, -0.25, 1.5, NaNs, NaN, tie, 0.5
    kinds = {(form, K) for form in ('labels', 'masks') for K in KS}
    assert {(w.split()[1], int(w.split()[2][2:])) for w in what} == kinds


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------------
def _five():
    rng = np.random.default_rng(801)
    frames = [_frame('blobs_noise', 9, 70, 'labels', 3, rng), _frame('blobs', 70, 33, 'masks', 3, rng), _frame('spiral', 40, 130, 'masks', 2, rng),
              _frame('serpentine', 65, 65, 'labels', 16, rng), _frame('ring', 1, 200, 'masks', 1, rng)]
    return [a for a, _ in frames], [i for _, i in frames]


def _names(answers, which, conn):
    return [P.names(P.slots(a, i), conn) for a, i in zip(answers, which)]


def test_one_call_for_five_mixed_frames_equals_five_calls():
    answers, which = _five()
    what = ['five[%d]' % i for i in range(5)]
    rule = dict(connectivity=8, min_area=3, largest_only=False, fill=0)
    together = _clean(answers, which, **rule)
    _assert_equal(together, answers, which, _names(answers, which, 8), what, **rule)
    host = together.cpu()[0]
    for i in range(5):
        alone = _clean(answers[i:i + 1], which[i:i + 1], **rule)
        assert torch.equal(alone.cpu()[0][0], host[i]) and torch.equal(alone.labels[0], together.labels[i]) and torch.equal(alone.components[0], together.components[i])


def test_two_calls_give_identical_bytes():
    a, i = _frame('blobs_noise', 480, 854, 'masks', 5, np.random.default_rng(802))
    given = _tensors([a], [i])
    rule = dict(connectivity=4, min_area=2, largest_only=False, fill=0)
    first = _clean([a], [i], given=given, **rule)
    second = _clean([a], [i], given=given, **rule)
    for x, y in zip(first.test_buffers, second.test_buffers):
        assert torch.equal(x, y)
    _assert_equal(first, [a], [i], _names([a], [i], 4), ['480x854 masks'], **rule)


def test_a_larger_out_is_written_only_where_it_should_be_and_components_false_touches_no_component():
    from frtm_vos_amd import ops
    answers, which = _five()
    rule = dict(connectivity=4, min_area=1, largest_only=True, fill=0)
    big = _clean(answers, which, pad=5000, **rule)                       # (_assert_equal checks every canary of the three buffers)
    _assert_equal(big, answers, which, _names(answers, which, 4), ['five'] * 5, **rule)
    # the same buffers again for two frames, without components: the component buffer keeps every byte
    before = big.test_buffers[1].clone()
    tensors, luts, ids = _tensors(answers[3:], which[3:])
    two = ops.clean_frames(tensors, luts=luts, ids=ids, out=big, components=False, **rule)
    assert two.comp_buf is None and two.components == [None, None] and two.label_buf.data_ptr() == big.label_buf.data_ptr()
    torch.cuda.synchronize()
    assert torch.equal(big.test_buffers[1], before)
    two.test_buffers = (big.test_buffers[0], torch.full_like(before, NAME), big.test_buffers[2])
    want = [P.clean(a, i, **rule) for a, i in zip(answers[3:], which[3:])]
    for k in range(2):
        assert np.array_equal(two.labels[k].cpu().numpy(), want[k][0]) and np.array_equal(two.cpu()[0][k].numpy(), want[k][2])
    assert two.ids(0) == tuple(int(v) for v in which[3]) and two.ids(1) == (0,)      # a label map's ids from the caller, a stack's from word 11


def test_a_row_that_leaves_its_buffer_raises_and_launches_nothing():
    from frtm_vos_amd import _hip as H
    answers, which = _five()
    tensors = [torch.from_numpy(a).to(DEV) for a in answers[:2]]
    id_bytes = [torch.from_numpy(i).to(DEV) for i in which[:2]]
    sizes = [(9, 70), (70, 33)]
    need = [(128 + 8 * h * w + 15) // 16 * 16 for h, w in sizes]
    labels = [torch.full((h * w,), BYTE, dtype=torch.uint8, device=DEV) for h, w in sizes]
    comps = [torch.full((h * w,), NAME, dtype=torch.int32, device=DEV) for h, w in sizes]
    work = [torch.full((b // 8,), WORD, dtype=torch.int64, device=DEV) for b in need]
    words = torch.full((2 * 193,), WORD, dtype=torch.int64, device=DEV)
    rows = [[0, 9, 70, tensors[0].data_ptr(), 9 * 70, 3, id_bytes[0].data_ptr(), 0,
             labels[0].data_ptr(), 9 * 70, comps[0].data_ptr(), 4 * 9 * 70, work[0].data_ptr(), need[0], 0, 0],
            [1, 70, 33, tensors[1].data_ptr(), 4 * 3 * 70 * 33, 3, id_bytes[1].data_ptr(), 0,
             labels[1].data_ptr(), 70 * 33 - 1, comps[1].data_ptr(), 4 * 70 * 33, work[1].data_ptr(), need[1], 0, 0]]      # one byte too few
    host = torch.tensor(rows, dtype=torch.int64)
    L = H.lib()
    assert L.frtm_clean_work_bytes(host.data_ptr(), 2) == sum(need)
    args = lambda dev: (host.data_ptr(), H.ptr(dev), 2, 8, 1, 0, 0, H.ptr(words), 2 * 192, H.ptr(words) + 8 * 2 * 192, 2)
    with pytest.raises(RuntimeError, match=r"frtm_clean_frames failed \(-1\).*frame 1's cleaned map \(2310 bytes\) leaves its 2309-byte buffer"):
        H.call('frtm_clean_frames', *args(host.to(DEV)))
    host[1, 9] += 1                                                      # the honest size
    for col, message in ((11, r"frame 1's component map \(9240 bytes\) leaves its 9239-byte buffer"), (13, "frame 1's work holds %d bytes, it needs %d" % (need[1] - 1, need[1])),
                         (4, r"frame 1's answer \(27720 bytes\) leaves its 27719-byte buffer")):
        host[1, col] -= 1
        with pytest.raises(RuntimeError, match=message):
            H.call('frtm_clean_frames', *args(host.to(DEV)))
        host[1, col] += 1
    torch.cuda.synchronize()
    for t, canary in [(x, BYTE) for x in labels] + [(x, NAME) for x in comps] + [(x, WORD) for x in work] + [(words, WORD)]:
        assert bool((t == canary).all())
    H.call('frtm_clean_frames', *args(host.to(DEV)))                     # the honest table is cleaned
    torch.cuda.synchronize()
    for k in range(2):
        want_labels, want_comp, want_words = P.clean(answers[k], which[k])
        h, w = sizes[k]
        assert np.array_equal(labels[k].cpu().numpy().reshape(h, w), want_labels) and np.array_equal(comps[k].cpu().numpy().reshape(h, w), want_comp)
        assert np.array_equal(words[192 * k:192 * (k + 1)].cpu().numpy().reshape(16, 12), want_words)
    assert words[384:].tolist() == [0, 0]


# ---- composition ----------------------------------------------------------------------------------------------------------------------------
def test_a_cleaned_answer_goes_into_describe_and_encode_as_it_is():
    from frtm_vos_amd import ops
    answers, which = _five()
    tensors, luts, ids = _tensors(answers, which)
    rule = dict(connectivity=8, min_area=4, largest_only=False, fill=0)
    plane_ids = [None if a.ndim == 2 else [int(v) for v in i] for a, i in zip(answers, which)]
    c = ops.clean_frames(tensors, luts=luts, ids=ids, plane_ids=plane_ids, **rule)
    assert c._host is None
    labels, out_ids = c.answers()
    assert c._host is None and out_ids == [tuple(int(v) for v in i) for i in which]      # every id was known on the host: no copy
    want = [P.clean(a, i, **rule)[0] for a, i in zip(answers, which)]
    report = ops.describe_frames(labels, ids=out_ids)
    assert np.array_equal(report.cpu().numpy(), O.report(want, which))
    coded = ops.encode_frames(labels, ids=out_ids, capacity=sum(len(i) * (a.shape[-2] * a.shape[-1] + 1) for a, i in zip(answers, which)))     # noise: more runs than the default holds
    for k in range(5):
        for oid, r in coded.rle(k).items():
            assert np.array_equal(ops.rle_decode(r['size'], r['counts']), want[k] == oid)
    raw = ops.describe_frames(tensors, luts=luts, ids=ids)
    assert torch.equal(c.cpu()[0][:, :, P.AREA], raw.cpu()[:, :, O.AREA])
    assert any((want[k] != (a if a.ndim == 2 else np.asarray(i, dtype=np.uint8)[P.slots(a, i)])).any() for k, (a, i) in enumerate(zip(answers, which)))


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
def test_tracker_clean_equals_the_reference(working_size):
    from frtm_vos_amd import ops
    size = BIG if working_size is not None else WS
    seq = _sequence('rt', 3, size, 2, 81)
    trk = _params(working_size).get_model().eval()
    with pytest.raises(ValueError, match='nothing was tracked'):
        trk.clean()
    torch.manual_seed(0)
    trk.initialize(seq[0][0], seq[0][1], seq[0][2])
    trk.current_frame += 1
    for image, _, _ in seq[1:]:
        masks = trk.track(image)
        trk.current_frame += 1
    answer = masks.cpu().numpy().copy()
    state = trk.current_masks.clone()
    lut = trk._object_lut().cpu().numpy()
    rule = dict(connectivity=8, min_area=9, largest_only=True, components=True)
    c = trk.clean(**rule)
    assert isinstance(c, ops.CleanedAnswers) and len(c) == 1 and c.K == [3] and c.sizes == [size] and tuple(answer.shape) == (3,) + size
    assert c._host is None and c.ids(0) == tuple(int(v) for v in lut) and c._host is None       # the tracker knows its object ids on the host
    want_labels, want_comp, want_words = P.clean(answer, lut, connectivity=8, min_area=9, largest_only=True)
    words, status = c.cpu()
    print('tracker answer %r: parts per slot %r, kept %r' % (size, words[0, :3, P.PARTS].tolist(), words[0, :3, P.KEPT].tolist()))
    assert status.tolist() == [0] and np.array_equal(words[0].numpy(), want_words)
    assert np.array_equal(c.labels[0].cpu().numpy(), want_labels) and np.array_equal(c.components[0].cpu().numpy(), want_comp)
    assert torch.equal(masks.cpu(), torch.from_numpy(answer)) and torch.equal(trk.current_masks, state)       # clean() reads the answer and leaves the state alone
    assert torch.equal(trk.describe().words[0, :, O.AREA].cpu(), words[0, :, P.AREA])
    again = trk.clean(out=c, **rule)
    assert again.label_buf.data_ptr() == c.label_buf.data_ptr() and np.array_equal(again.labels[0].cpu().numpy(), want_labels)
    plain = trk.clean()
    assert plain.components == [None] and np.array_equal(plain.labels[0].cpu().numpy(), lut[P.slots(answer, lut)])
    if working_size is not None:
        assert trk.native_labels is not None and tuple(trk.native_labels.shape) == (1,) + BIG and tuple(trk.current_masks.shape[-2:]) == WS
        assert np.array_equal(plain.labels[0].cpu().numpy(), trk.native_labels.cpu().numpy()[0])


def test_pool_clean_is_one_call_for_all_streams():
    streams = [_sequence('pa', 3, WS, 1, 90), _sequence('pb', 3, WS, 2, 91), _sequence('pc', 3, BIG, 2, 92), _sequence('pd', 3, (192, 224), 3, 93)]
    pool = _params().get_stream_pool(max_streams=4, working_size=WS)
    with pytest.raises(ValueError, match='StreamPool.clean: no stream has an answer'):
        pool.clean()
    sids = [pool.open() for _ in streams]
    counters = lambda: (pool.trunk_passes, pool.frame_launches, pool.refiner_passes, pool.grouped_launches, pool.render_launches, pool.describe_launches,
                        pool.encode_launches)
    per_tick = []
    for t in range(3):
        frames = {}
        for sid, seq in zip(sids, streams):
            image, labels, new_objects = seq[t]
            if len(new_objects) > 0:
                torch.manual_seed(0)
                pool.initialize(sid, image, labels, new_objects)
            frames[sid] = image
        start = counters()
        out = pool.step(frames)
        per_tick.append(tuple(b - a for a, b in zip(start, counters())))
        if t == 1:                                                       # a clean() between two ticks: the next tick makes the launches it made before
            pool.clean(min_area=4)
    assert per_tick[1] == per_tick[2] and pool.clean_launches == 1
    before = counters()
    index, c = pool.clean(connectivity=4, min_area=6, components=True)
    assert pool.clean_launches == 2 and sorted(index) == sorted(sids) and sorted(index.values()) == [0, 1, 2, 3] and len(c) == 4
    assert counters() == before
    order = sorted(sids, key=lambda sid: index[sid])
    answers = [out[sid].cpu().numpy() for sid in order]
    luts = [pool.tracker(sid)._object_lut().cpu().numpy() for sid in order]
    assert c.K == [a.shape[0] for a in answers] and sorted(c.K) == [2, 3, 3, 4] and len(set(c.sizes)) == 3
    words, status = c.cpu()
    assert status.tolist() == [0, 0, 0, 0]
    for k, (a, lut) in enumerate(zip(answers, luts)):
        want_labels, want_comp, want_words = P.clean(a, lut, connectivity=4, min_area=6)
        assert np.array_equal(words[k].numpy(), want_words) and np.array_equal(c.labels[k].cpu().numpy(), want_labels)
        assert np.array_equal(c.components[k].cpu().numpy(), want_comp) and c.ids(k) == tuple(int(v) for v in lut)
        assert torch.equal(out[order[k]].cpu(), torch.from_numpy(a))       # the answers are read, not written
    some, c2 = pool.clean([sids[3], sids[0]], out=c, connectivity=4, min_area=6)
    assert pool.clean_launches == 3 and some == {sids[3]: 0, sids[0]: 1} and c2.label_buf.data_ptr() == c.label_buf.data_ptr()
    assert torch.equal(c2.cpu()[0][0], words[index[sids[3]]]) and torch.equal(c2.cpu()[0][1], words[index[sids[0]]])
    assert counters() == before
    with pytest.raises(KeyError):
        pool.clean([12345])
    for sid in sids:
        pool.close(sid)
