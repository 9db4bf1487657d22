"""The cleaning of an answer without a GPU (csrc/object_parts.hip, ops.clean_frames / CleanedAnswers): the numpy statement of
tests/_parts_refs.py against a flood fill over pixels and against scipy.ndimage.label, the ABI and its constants, frtm_clean_work_bytes, the
refusals of the C entries (they run on the host, before anything is enqueued) and of the wrapper, CleanedAnswers' host logic and the kernels'
scratch / spill / LDS budget.  The kernels themselves are checked on the GPU (tests/test_object_parts_gpu.py).  Everything is an integer: all
comparisons are equalities."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _parts_refs as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
ENTRY = 'frtm_clean_frames'
FRTM_ERR_ARG = -1
SIZES = [(1, 1), (1, 9), (7, 1), (2, 2), (5, 8), (17, 13), (33, 40), (40, 33)]


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read(), flags=re.S)


def _define(name):
    return int(re.search(r'#define\s+%s\s+(\d+)' % name, _header()).group(1))


def test_abi_declares_exports_and_binds_the_entry_points():
    from frtm_vos_amd import _hip, build, ops
    hdr = _header()
    assert re.search(r'\bint\s+%s\s*\(' % ENTRY, hdr) and hasattr(_hip.lib(), ENTRY)
    assert re.search(r'\bsize_t\s+frtm_clean_work_bytes\s*\(', hdr) and hasattr(_hip.lib(), 'frtm_clean_work_bytes')
    res, args = _hip.SIGNATURES[ENTRY]
    assert res is _hip.I and len(args) == 12                            # two tables, n, four rule scalars, words + count, status + count, stream
    assert args[4] is ctypes.c_longlong                                 # min_area reaches 2^28 and is a 64-bit word
    assert _hip.SIGNATURES['frtm_clean_work_bytes'] == (ctypes.c_size_t, [_hip.P, _hip.I])
    assert 'object_parts.hip' in build.SOURCES
    assert _define('FRTM_PARTS_ROW_WORDS') == ops.PARTS_ROW_WORDS == 16 and ops.PARTS_ROW_WORDS >= ops.OBJECT_ROW_WORDS + 6
    assert _define('FRTM_PARTS_WORDS') == ops.PARTS_WORDS == P.WORDS == 12
    assert _define('FRTM_PARTS_TILE_H') == ops.PARTS_TILE_H and _define('FRTM_PARTS_TILE_W') == ops.PARTS_TILE_W
    assert ops.OBJECT_SLOTS == P.SLOTS == 16
    src = open(os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'object_parts.hip')).read()
    assert '#include "object_rows.h"' in src and 'int ob_check(' not in src and '#include "parts_core.h"' in src


# ---- the two restatements, and scipy ------------------------------------------------------------------------------------------------------
def _pictures(h, w, rng):
    for what in P.PICTURES:
        yield what, P.picture(what, h, w, o=1, o2=2, tile=(3, 4), rng=rng)
    blobs = rng.integers(0, 4, (h, w))
    yield 'blobs with holes', np.where(rng.random((h, w)) < 0.2, -1, blobs)


def test_numpy_names_equal_the_flood_fill_on_every_picture():
    rng = np.random.default_rng(21)
    seen = 0
    for h, w in SIZES:
        for what, slot in _pictures(h, w, rng):
            for conn in (4, 8):
                a, b = P.names(slot, conn), P.parts_loop(slot, conn)
                assert np.array_equal(a, b), (what, h, w, conn)
                assert ((a >= 0) == (slot >= 0)).all() and (a.reshape(-1)[a.reshape(-1) >= 0] <= np.flatnonzero(a.reshape(-1) >= 0)).all()
                seen += 1
    assert seen == len(SIZES) * (len(P.PICTURES) + 1) * 2


def test_the_pictures_have_the_parts_they_are_made_for():
    rng = np.random.default_rng(22)
    count = lambda slot, conn, s=1: len(np.unique(P.names(slot, conn)[slot == s]))
    board = P.picture('checker', 6, 7)
    assert count(board, 4) == 21 and count(board, 8) == 1 and count(board, 8, 0) == 1 and count(board, 4, 0) == 21
    line = P.picture('diagonal', 9, 12)
    assert count(line, 8) == 1 and count(line, 4) == 9
    for h, w in ((9, 9), (21, 34), (40, 40), (12, 7)):
        spiral = P.picture('spiral', h, w)
        assert count(spiral, 4) == 1 and count(spiral, 8) == 1, (h, w)
    assert (P.picture('spiral', 40, 40) == 1).sum() > 40 * 40 // 2 - 40       # one path about h w / 2 long
    for what in ('comb', 'comb_mirrored', 'serpentine'):
        assert count(P.picture(what, 11, 15), 4) == 1, what
    assert count(P.picture('comb', 11, 15), 4, 0) == 7 and count(P.picture('serpentine', 11, 15), 4, 0) == 5
    ring = P.picture('ring', 40, 40, o=1, o2=2)
    assert count(ring, 8, 1) == 1 and count(ring, 8, 2) == 1 and count(ring, 4, 0) == 2       # the background inside the ring is a part of its own
    equal = np.array([0, 5], dtype=np.uint8)[P.picture('equal', 10, 10)]
    labels, comp, words = P.clean(equal, [0, 5], largest_only=True)
    assert words[1, P.PARTS] == 2 and words[1, P.KEPT] == 1 and words[1, P.LARGEST_NAME] == 0 and words[1, P.LARGEST_AREA] == 6
    assert words[1, P.X_MIN:P.Y_MAX + 1].tolist() == [0, 0, 1, 2] and (labels[:3, :2] == 5).all() and (labels[7:, 8:] == 0).all()
    assert count(P.picture('noise', 40, 40, rng=rng), 4) > 50


def test_the_numpy_statement_follows_the_contract_on_hand_made_frames():
    labels = np.array([[4, 4, 0, 9, 9],
                       [0, 0, 0, 0, 9],
                       [4, 0, 7, 0, 0],
                       [4, 4, 0, 0, 9]], dtype=np.uint8)
    out, comp, words = P.clean(labels, [0, 4, 9], connectivity=4, min_area=3)
    assert comp.tolist() == [[0, 0, 2, 3, 3], [2, 2, 2, 2, 3], [10, 2, -1, 2, 2], [10, 10, 2, 2, 19]] and comp.dtype == np.int32
    assert out.tolist() == [[0, 0, 0, 9, 9], [0, 0, 0, 0, 9], [4, 0, 7, 0, 0], [4, 4, 0, 0, 0]] and out.dtype == np.uint8     # 7 is not listed: kept as it is
    assert words[0].tolist() == [1, 1, 10, 10, 10, 2, 0, 0, 4, 3, 0, 0]        # the background: unruled, counted, kept
    assert words[1].tolist() == [2, 1, 5, 3, 3, 10, 0, 2, 1, 3, 1, 4]
    assert words[2].tolist() == [2, 1, 4, 3, 3, 3, 3, 0, 4, 1, 1, 9] and not words[3:].any()
    # 8-connectivity joins the background diagonally around the unlisted pixel, and nothing else here
    assert np.array_equal(P.clean(labels, [0, 4, 9], connectivity=8)[1], P.parts_loop(P.slots(labels, [0, 4, 9]), 8))
    # fill = 9 makes slot 2 the unruled one and rules the background
    out, _, words = P.clean(labels, [0, 4, 9], connectivity=4, min_area=3, fill=9)
    assert words[:3, P.RULED].tolist() == [1, 1, 0] and words[2, P.KEPT] == 2 and words[1, P.KEPT] == 1
    assert out.tolist() == [[9, 9, 0, 9, 9], [0, 0, 0, 0, 9], [4, 0, 7, 0, 0], [4, 4, 0, 0, 9]]
    # an empty slot: -1 and the empty box
    _, _, words = P.clean(labels, [0, 200])
    assert words[1].tolist() == [0, 0, 0, 0, 0, -1, 5, 4, -1, -1, 1, 200]
    # a stack: the decode's hand-placed pixels
    stack = np.zeros((3, 1, 8), dtype=np.float32)
    stack[1, 0, :6] = [0.5, 0.50001, 0.75, 1.5, -0.25, np.nan]
    stack[2, 0, 2], stack[2, 0, 5] = 0.75, 0.625
    stack[:, 0, 6] = [0.9, 0.75, 0.8]
    stack[:, 0, 7] = np.nan
    out, comp, words = P.clean(stack, [0, 5, 9], connectivity=4)
    assert comp.tolist() == [[0, 1, 1, 1, 4, 5, 6, 6]] and out.tolist() == [[0, 5, 5, 5, 0, 9, 0, 0]]
    assert words[:3, P.PARTS].tolist() == [3, 1, 1] and words[0, P.LARGEST_NAME] == 6 and words[0, P.AREA] == 4
    identity = P.clean(stack, [0, 5, 9], min_area=1)[0]
    assert np.array_equal(identity, np.array([0, 5, 9], dtype=np.uint8)[P.slots(stack, [0, 5, 9])])


def test_the_partition_equals_scipy_label():
    ndimage = pytest.importorskip('scipy.ndimage')
    rng = np.random.default_rng(23)
    for h, w in SIZES:
        for what, slot in _pictures(h, w, rng):
            for conn, structure in ((4, [[0, 1, 0], [1, 1, 1], [0, 1, 0]]), (8, np.ones((3, 3), dtype=int))):
                ours = P.names(slot, conn)
                for s in range(int(slot.max()) + 1):
                    theirs, count = ndimage.label(slot == s, structure=structure)
                    mine = np.where(slot == s, ours, -1)
                    assert np.array_equal(P.partition_of(theirs), mine), (what, h, w, conn, s)
                    assert count == len(np.unique(mine[mine >= 0]))


def test_the_rule_in_numpy_equals_the_rule_on_the_flood_fill():
    rng = np.random.default_rng(24)
    for h, w in ((9, 14), (33, 40)):
        for what, slot in _pictures(h, w, rng):
            ids = [0, 7, 3, 250]
            labels = np.where(slot >= 0, np.asarray(ids)[np.maximum(slot, 0)], 99).astype(np.uint8)
            for conn, min_area, largest, fill in ((4, 1, False, 0), (8, 5, False, 0), (4, 1, True, 0), (8, 5, True, 7)):
                a = P.clean(labels, ids, conn, min_area, largest, fill)
                b = P.clean(labels, ids, conn, min_area, largest, fill, part_names=P.parts_loop(slot, conn))
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (what, h, w, conn)
                out, comp, words = a
                if min_area == 1 and not largest:
                    assert np.array_equal(out, labels)                  # the identity on slots
                assert (words[:4, P.AREA] == [(slot == s).sum() for s in range(4)]).all() and (out[slot < 0] == 99).all()
                assert (words[:4, P.KEPT_AREA] == [((slot == s) & (out == ids[s])).sum() if ids[s] != fill else (slot == s).sum() for s in range(4)]).all()


# ---- the C entries: addresses that are never followed ------------------------------------------------------------------------------------
ANS, IDS, LABELS, COMPS, WORK, WORDS, STATUS = 0x300000, 0x400000, 0x500000, 0x600000, 0x700000, 0x800000, 0x900000
KEYS = ['form', 'h', 'w', 'ans', 'ans_bytes', 'K', 'ids', 'zero', 'labels', 'labels_bytes', 'comps', 'comps_bytes', 'work', 'work_bytes', 'zero0', 'zero1']


def _need(h, w):
    return (128 + 8 * h * w + 15) // 16 * 16


def _row(**kw):
    """A valid row: a 7 x 13 stack of K = 3 planes with every output."""
    row = dict(form=1, h=7, w=13, ans=ANS, ans_bytes=4 * 3 * 7 * 13, K=3, ids=IDS, zero=0, labels=LABELS, labels_bytes=91, comps=COMPS,
               comps_bytes=4 * 91, work=WORK, work_bytes=_need(7, 13), zero0=0, zero1=0)
    row.update(kw)
    return [row[k] for k in KEYS]


def _table(rows):
    return (ctypes.c_longlong * (16 * len(rows)))(*[int(v) for r in rows for v in r])


def _work_bytes(rows, n=None):
    from frtm_vos_amd import _hip
    L = _hip.lib()
    t = _table(rows)
    got = L.frtm_clean_work_bytes(ctypes.addressof(t), len(rows) if n is None else n)
    return got, L.frtm_last_error().decode()


def _call(rows, n=None, host=True, dev=True, conn=8, min_area=1, largest=0, fill=0, words=WORDS, word_count=None, status=STATUS, status_count=None):
    from frtm_vos_amd import _hip
    L = _hip.lib()
    t = _table(rows)
    n = len(rows) if n is None else n
    rc = L.frtm_clean_frames(ctypes.addressof(t) if host else None, ctypes.addressof(t) if dev else None, n, conn, min_area, largest, fill, words,
                             16 * 12 * max(n, 0) if word_count is None else word_count, status, max(n, 0) if status_count is None else status_count, None)
    return rc, L.frtm_last_error().decode()


LABEL_MAP = dict(form=0, ans_bytes=7 * 13, K=2)
REFUSED_BY_OB_CHECK = [
    (dict(form=2), 'answer form 2'), (dict(zero=1), 'last word 1'), (dict(h=0), 'size 0 x 13'), (dict(w=16385, ans_bytes=1 << 40), 'size 7 x 16385'),
    (dict(K=0), 'K = 0 slots'), (dict(LABEL_MAP, K=17), 'K = 17 slots'), (dict(ans=0), 'null address .answer 0,'), (dict(ids=0), r'null address .*ids 0\)'),
    (dict(ans_bytes=4 * 3 * 7 * 13 - 1), r'answer \(1092 bytes\) leaves its 1091-byte buffer'), (dict(ans_bytes=-1), 'answer_bytes -1 is not a size'),
    (dict(ans=ANS + 2), 'stack at 0x300002 is not 4-byte aligned'),
]
REFUSED_OUTPUTS = [
    (dict(zero0=1), r'last words 1, 0'), (dict(zero1=-1), r'last words 0, -1'), (dict(labels=0), 'null address .labels 0,'), (dict(work=0), r'null address .*work 0\)'),
    (dict(labels_bytes=90), r'cleaned map \(91 bytes\) leaves its 90-byte buffer'), (dict(labels_bytes=-1), 'is not a size'),
    (dict(comps_bytes=1 << 47), 'is not a size'), (dict(labels=ANS + 1000), 'cleaned map at 0x3003e8 overlaps its answer at 0x300000'),
    (dict(LABEL_MAP, labels=ANS - 90), 'overlaps its answer'), (dict(comps=COMPS + 2), 'component map at 0x600002 is not 4-byte aligned'),
    (dict(comps_bytes=4 * 91 - 1), r'component map \(364 bytes\) leaves its 363-byte buffer'), (dict(work=WORK + 8), 'work at 0x700008 is not 16-byte aligned'),
    (dict(work_bytes=_need(7, 13) - 1), 'work holds %d bytes, it needs %d' % (_need(7, 13) - 1, _need(7, 13))),
]


@pytest.mark.parametrize('change,message', REFUSED_BY_OB_CHECK, ids=[m for _, m in REFUSED_BY_OB_CHECK])
def test_rows_ob_check_refuses_are_refused_by_both_entries(change, message):
    rows = [_row(), _row(**change)]
    rc, msg = _call(rows)
    assert rc == FRTM_ERR_ARG and ENTRY in msg and 'frame 1' in msg and re.search(message, msg), msg
    size, msg = _work_bytes(rows)
    assert size == 0 and 'frtm_clean_work_bytes' in msg and 'frame 1' in msg and re.search(message, msg), msg


@pytest.mark.parametrize('change,message', REFUSED_OUTPUTS, ids=[m for _, m in REFUSED_OUTPUTS])
def test_bad_outputs_are_refused_before_anything_is_enqueued(change, message):
    rows = [_row(), _row(), _row(**change)]
    rc, msg = _call(rows)
    assert rc == FRTM_ERR_ARG and ENTRY in msg and 'frame 2' in msg and re.search(message, msg), msg
    assert _work_bytes(rows)[0] == 3 * _need(7, 13)                     # the work size reads the first 8 words of a row only


def test_bad_calls_are_refused_before_anything_is_enqueued():
    for kw, message in ((dict(n=0), 'n = 0'), (dict(n=-1), 'n = -1'), (dict(n=65536), 'n = 65536'), (dict(host=False), 'null table'), (dict(dev=False), 'null table'),
                        (dict(words=None), 'null words or status'), (dict(status=None), 'null words or status'), (dict(words=WORDS + 4), '8-byte aligned'),
                        (dict(status=STATUS + 2), '8-byte aligned'), (dict(word_count=191), 'words holds 191 words, 1 frames need 192'),
                        (dict(status_count=0), 'status holds 0 words, 1 frames need 1'),
                        (dict(conn=6), 'connectivity = 6 (4 or 8)'), (dict(conn=0), 'connectivity = 0'), (dict(min_area=0), 'min_area = 0 (1 .. 2^28)'),
                        (dict(min_area=(1 << 28) + 1), 'min_area = %d' % ((1 << 28) + 1)), (dict(min_area=-5), 'min_area = -5'),
                        (dict(largest=2), 'largest_only = 2 (0 or 1)'), (dict(largest=-1), 'largest_only = -1'), (dict(fill=256), 'fill = 256 (0 .. 255)'),
                        (dict(fill=-1), 'fill = -1')):
        rc, msg = _call([_row()], **kw)
        assert rc == FRTM_ERR_ARG and ENTRY in msg and message in msg, (kw, msg)
    # a row without a component map is a good row: what is refused next is the words
    rc, msg = _call([_row(comps=0, comps_bytes=0)], word_count=1)
    assert rc == FRTM_ERR_ARG and 'words holds 1 words' in msg, msg
    for kw, message in ((dict(n=0), 'n = 0'), (dict(n=65536), 'n = 65536')):
        size, msg = _work_bytes([_row()], **kw)
        assert size == 0 and 'frtm_clean_work_bytes' in msg and message in msg, (kw, msg)
    from frtm_vos_amd import _hip
    assert _hip.lib().frtm_clean_work_bytes(None, 1) == 0 and 'null table' in _hip.lib().frtm_last_error().decode()


def test_work_bytes_equals_the_formula_of_the_header():
    from frtm_vos_amd import ops
    for h, w in ((1, 1), (1, 3), (7, 13), (480, 854), (1080, 1920), (16384, 16384)):
        for row in (_row(h=h, w=w, ans_bytes=1 << 45), _row(form=0, K=16, h=h, w=w, ans_bytes=1 << 45)):
            size, msg = _work_bytes([row])
            assert size == _need(h, w) == ops.clean_work_bytes(h, w) and size % 16 == 0 and size >= 128 + 8 * h * w, msg
    mixed, _ = _work_bytes([_row(h=10, w=10, ans_bytes=1 << 45), _row(h=1080, w=1920, ans_bytes=1 << 45), _row(h=1, w=1)])
    assert mixed == _need(10, 10) + _need(1080, 1920) + _need(1, 1) == 928 + 16588928 + 144


# ---- CleanedAnswers and the wrapper -----------------------------------------------------------------------------------------------------------
def _host_answers(frames, ids, components=True, plane_ids=None, **rule):
    from frtm_vos_amd import ops
    sizes = [f.shape[-2:] for f in frames]
    pixels = sum((h * w + 15) // 16 * 16 for h, w in sizes)
    label_buf, comp_buf = torch.full((pixels + 5,), 77, dtype=torch.uint8), torch.full((pixels + 5,), -7, dtype=torch.int32)
    n = len(frames)
    word_buf = torch.zeros(n * 193 + 3, dtype=torch.int64)
    o = 0
    for i, (f, idv) in enumerate(zip(frames, ids)):
        h, w = sizes[i]
        labels, comp, words = P.clean(f, idv, **rule)
        label_buf[o:o + h * w] = torch.from_numpy(labels.reshape(-1))
        comp_buf[o:o + h * w] = torch.from_numpy(comp.reshape(-1))
        word_buf[192 * i:192 * (i + 1)] = torch.from_numpy(words.reshape(-1))
        o += (h * w + 15) // 16 * 16
    return ops.CleanedAnswers(label_buf, comp_buf if components else None, word_buf, sizes, [len(v) for v in ids],
                              ids if plane_ids is None else plane_ids)


def test_cleaned_answers_host_logic():
    from frtm_vos_amd import ops
    a = np.array([[4, 4, 0, 9, 9], [0, 0, 0, 0, 9], [4, 0, 7, 0, 0], [4, 4, 0, 0, 9]], dtype=np.uint8)
    b = P.picture('equal', 6, 7).astype(np.uint8)
    c = _host_answers([a, b], [[0, 4, 9], [0, 1, 200]], connectivity=4, min_area=3)
    assert len(c) == 2 and c.offsets == [0, 32] and c.words.shape == (2, 16, 12) and c.status.shape == (2,)
    assert c.labels[0].shape == (4, 5) and c.labels[1].shape == (6, 7) and c.components[1].dtype == torch.int32
    assert c.labels[0].tolist() == [[0, 0, 0, 9, 9], [0, 0, 0, 0, 9], [4, 0, 7, 0, 0], [4, 4, 0, 0, 0]]
    assert c.cpu() is c.cpu() and c.cpu()[0].shape == (2, 16, 12)
    assert c.objects(0) == {0: ops.PartStats(1, 1, 10, 10, 10, (0, 0, 4, 3), 2, False), 4: ops.PartStats(2, 1, 5, 3, 3, (0, 2, 1, 3), 10, True),
                            9: ops.PartStats(2, 1, 4, 3, 3, (3, 0, 4, 1), 3, True)}
    assert c.objects(1)[200] == ops.PartStats(0, 0, 0, 0, 0, None, None, True) and c.objects(1)[1].parts == 2
    assert c.ids(0) == (0, 4, 9) and c.ids(1) == (0, 1, 200)
    labels, ids = c.answers()
    assert ids == [(0, 4, 9), (0, 1, 200)] and all(x is y for x, y in zip(labels, c.labels))
    # ids the caller did not name on the host come from word 11
    unknown = _host_answers([a], [[0, 4, 9]], plane_ids=[None])
    assert unknown._host is None and unknown.ids(0) == (0, 4, 9) and unknown._host is not None
    assert _host_answers([a], [[0, 4, 9]], components=False).components == [None]
    # a status that is not 0 raises, naming the frame -- every time
    c.word_buf[2 * 192 + 1] = 2
    c._host = None
    for _ in range(2):
        with pytest.raises(RuntimeError, match='frame 1 has status 2'):
            c.objects(0)
    words = torch.zeros(193, dtype=torch.int64)
    with pytest.raises(TypeError, match='1-d int64'):
        ops.CleanedAnswers(torch.zeros(16, dtype=torch.uint8), None, words.int(), [(2, 2)], [1], [None])
    with pytest.raises(TypeError, match='1-d int64'):
        ops.CleanedAnswers(torch.zeros(16, dtype=torch.uint8), None, words[:192], [(2, 2)], [1], [None])
    with pytest.raises(TypeError, match='1-d uint8'):
        ops.CleanedAnswers(torch.zeros(16, dtype=torch.int32), None, words, [(2, 2)], [1], [None])
    with pytest.raises(TypeError, match='1-d int32 tensor or None'):
        ops.CleanedAnswers(torch.zeros(16, dtype=torch.uint8), torch.zeros(16), words, [(2, 2)], [1], [None])
    with pytest.raises(ValueError, match='1 sizes, 2 slot counts'):
        ops.CleanedAnswers(torch.zeros(16, dtype=torch.uint8), None, words, [(2, 2)], [1, 1], [None])
    with pytest.raises(ValueError, match='need 32 packed pixels, the buffers hold 16'):
        ops.CleanedAnswers(torch.zeros(16, dtype=torch.uint8), None, words, [(4, 5)], [1], [None])


def test_clean_frames_refuses_before_any_launch():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from frtm_vos_amd import ops
    cpu = torch.zeros(4, 6, dtype=torch.uint8)
    with pytest.raises(ValueError, match='clean_frames: 0 frames'):
        ops.clean_frames([])
    with pytest.raises(RuntimeError, match='clean_frames: answer 0 is on cpu.*no CPU fallback'):
        ops.clean_frames([cpu], ids=[[1, 2]])
    for bad in (cpu.float(), torch.zeros(2, 4, 6, dtype=torch.float64), torch.zeros(1, 4, 6, dtype=torch.uint8), 'labels', None):
        with pytest.raises(TypeError, match='clean_frames: answer 0 is a .* label map or a'):
            ops.clean_frames([bad], ids=[[1]])
    for bad in (None, 7, [1.0], [True]):
        with pytest.raises(TypeError, match=r'clean_frames: .*ids'):
            ops.clean_frames([cpu], ids=[bad])
    with FakeTensorMode():
        labels = torch.empty(4, 6, dtype=torch.uint8, device='cuda')
        stack = torch.empty(2, 4, 6, device='cuda')
        lut = torch.empty(2, dtype=torch.uint8, device='cuda')
        small = (torch.empty(32, dtype=torch.uint8, device='cuda'), torch.empty(32, dtype=torch.int32, device='cuda'),
                 torch.empty(193, dtype=torch.int64, device='cuda'))
    with pytest.raises(TypeError, match=r'needs luts\[0\]'):
        ops.clean_frames([stack])
    for kw, message in ((dict(connectivity=6), 'connectivity is 4 or 8, got 6'), (dict(connectivity=0), 'connectivity is 4 or 8'),
                        (dict(min_area=0), r'min_area is 1 .. 2\^28, got 0'), (dict(min_area=(1 << 28) + 1), 'min_area is 1'),
                        (dict(fill=256), 'fill is 0 .. 255, got 256'), (dict(fill=-1), 'fill is 0 .. 255'), (dict(largest_only=2), 'largest_only is a bool')):
        with pytest.raises(ValueError, match=message):
            ops.clean_frames([labels], ids=[[1]], **kw)
    for kw in (dict(connectivity=8.0), dict(min_area='5'), dict(fill=True), dict(min_area=2.5)):
        with pytest.raises(TypeError, match='is an int'):
            ops.clean_frames([labels], ids=[[1]], **kw)
    with pytest.raises(ValueError, match='1 answers, 2 plane_ids'):
        ops.clean_frames([stack], luts=[lut], plane_ids=[[0, 1], [0, 1]])
    with pytest.raises(ValueError, match=r'plane_ids\[0\] lists 3 ids, the stack has 2 planes'):
        ops.clean_frames([stack], luts=[lut], plane_ids=[[0, 1, 2]])
    with pytest.raises(TypeError, match='out is an ops.CleanedAnswers'):
        ops.clean_frames([labels], ids=[[1]], out=small[0])
    out = ops.CleanedAnswers(small[0], small[1], small[2], [(4, 6)], [1], [(1,)])
    with pytest.raises(ValueError, match='out holds 32 pixels and 193 words, 2 frames need 64 and 386'):
        ops.clean_frames([labels, labels], ids=[[1], [2]], out=out)
    with pytest.raises(ValueError, match='out holds no component maps'):
        ops.clean_frames([labels], ids=[[1]], components=True, out=ops.CleanedAnswers(small[0], None, small[2], [(4, 6)], [1], [(1,)]))
    host = ops.CleanedAnswers(torch.zeros(32, dtype=torch.uint8), None, torch.zeros(193, dtype=torch.int64), [(4, 6)], [1], [(1,)])
    with pytest.raises(RuntimeError, match='out is on cpu.*no CPU fallback'):
        ops.clean_frames([labels], ids=[[1]], out=host)


def test_clean_shares_the_checks_and_tracker_and_pool_have_the_surface():
    from frtm_vos_amd import ops
    from frtm_vos_amd.model.stream_pool import StreamPool
    from frtm_vos_amd.model.tracker import Tracker
    src = inspect.getsource(ops.clean_frames)
    assert '_object_frames(' in src and '_object_table(' in src and 'synchronize' not in src and '.cpu()' not in src and '.item()' not in src
    assert list(inspect.signature(ops.clean_frames).parameters) == ['answers', 'luts', 'ids', 'connectivity', 'min_area', 'largest_only', 'fill',
                                                                    'components', 'plane_ids', 'out']
    assert [p.default for p in inspect.signature(ops.clean_frames).parameters.values()][1:] == [None, None, 8, 1, False, 0, False, None, None]
    assert list(inspect.signature(Tracker.clean).parameters) == ['self', 'out', 'rule']
    assert list(inspect.signature(StreamPool.clean).parameters) == ['self', 'sids', 'out', 'rule']
    for fn in (Tracker.clean, StreamPool.clean):
        src = inspect.getsource(fn)
        assert 'plane_ids' in src and 'current_masks =' not in src and 'native_labels[' not in src       # the answer is read, no state is written
    assert 'describe_answer' in inspect.getsource(Tracker.clean) and "_answers('clean'" in inspect.getsource(StreamPool.clean)
    assert 'clean_launches' in inspect.getsource(StreamPool.__init__)


# ---- the kernels' budget -----------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_and_spill_nothing():
    assert os.path.exists(HIPCC), 'hipcc is needed (the build needs it as well)'
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'object_parts.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'object_parts.hip')], check=True, capture_output=True, cwd=d)
        isa = open(out).read()
    blocks = [b for b in re.split(r'\n  - \.agpr_count:', isa) if '.name:' in b and 'k_parts_' in b]
    names = sorted(re.search(r'\.name:\s+(\S+)', b).group(1) for b in blocks)
    assert len(blocks) == 6 and all(any(k in n for n in names) for k in ('begin', 'local', 'seam', 'flatten', 'slots', 'write')), names
    for b in blocks:
        field = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, b).group(1))
        print('%s: %d VGPRs, %d SGPRs, %d bytes of LDS' % (re.search(r'\.name:\s+(\S+)', b).group(1), field('vgpr_count'), field('sgpr_count'),
                                                           field('group_segment_fixed_size')))
        assert field('vgpr_spill_count') == 0 and field('sgpr_spill_count') == 0 and field('private_segment_fixed_size') == 0
        assert field('group_segment_fixed_size') <= 40 * 1024              # four workgroups per CU
        assert not re.search(r'\.uses_dynamic_stack:\s+true', b)
    assert 'atomic_add_f' not in isa and 'atomic_fadd' not in isa and 'atomic_pk_add' not in isa     # integer atomics only
