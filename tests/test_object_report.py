"""The object report without a GPU (csrc/object_report.hip, ops.describe_frames / ObjectReport): the ABI, the refusals of the C entry (they
run on the host, before anything is enqueued), the numpy statement of tests/_object_refs.py against a plain loop over pixels, ObjectReport's
host logic, the wrapper's refusals and the kernel's scratch / spill / LDS budget.  The kernel itself is checked on the GPU
(tests/test_object_report_gpu.py).  Every word is an integer: all comparisons are equalities."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest
import torch

import _object_refs as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
ENTRY = 'frtm_describe_frames'
FRTM_ERR_ARG = -1


def test_abi_declares_exports_and_binds_the_entry_point():
    from frtm_vos_amd import _hip, build, ops
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+%s\s*\(' % ENTRY, hdr) and hasattr(_hip.lib(), ENTRY)
    res, args = _hip.SIGNATURES[ENTRY]
    assert res is _hip.I and len(args) == 6                            # two tables, n, out, out_words, stream
    assert 'object_report.hip' in build.SOURCES
    macros = {k: int(v) for k, v in re.findall(r'#define\s+FRTM_OBJECT_(\w+)\s+(\d+)', hdr)}
    assert macros == dict(LABELS=ops.OBJECT_ANSWERS['labels'], MASKS=ops.OBJECT_ANSWERS['masks'], ROW_WORDS=ops.OBJECT_ROW_WORDS,
                          SLOTS=ops.OBJECT_SLOTS, WORDS=ops.OBJECT_WORDS)
    assert (macros['LABELS'], macros['MASKS'], macros['ROW_WORDS'], macros['SLOTS'], macros['WORDS']) == (0, 1, 8, O.SLOTS, O.WORDS) == (0, 1, 8, 16, 12)


# ---- refusals of the C entry: addresses that are never followed -----------------------------------------------------------------------
ANS, IDS, OUT = 0x300000, 0x400000, 0x500000
KEYS = ['form', 'h', 'w', 'ans', 'ans_bytes', 'K', 'ids', 'zero']


def _row(**kw):
    """A valid row: a 7 x 13 stack of K = 3 planes."""
    row = dict(form=1, h=7, w=13, ans=ANS, ans_bytes=4 * 3 * 7 * 13, K=3, ids=IDS, zero=0)
    row.update(kw)
    return [row[k] for k in KEYS]


def _call(rows, n=None, host=True, dev=True, out=OUT, out_words=None):
    from frtm_vos_amd import _hip
    L = _hip.lib()
    t = (ctypes.c_longlong * (8 * len(rows)))(*[int(v) for r in rows for v in r])
    n = len(rows) if n is None else n
    rc = L.frtm_describe_frames(ctypes.addressof(t) if host else None, ctypes.addressof(t) if dev else None, n, out,
                                16 * 12 * max(n, 0) if out_words is None else out_words, None)
    return rc, L.frtm_last_error().decode()


LABELS = dict(form=0, ans_bytes=7 * 13, K=2)
REFUSED = [
    (dict(form=2), 'answer form 2'), (dict(form=-1), 'answer form -1'), (dict(zero=1), 'last word 1'),
    (dict(h=0), 'size 0 x 13'), (dict(w=0), 'size 7 x 0'), (dict(h=16385, ans_bytes=1 << 40), 'size 16385 x 13'), (dict(w=16385, ans_bytes=1 << 40), 'size 7 x 16385'),
    (dict(K=0), 'K = 0 slots'), (dict(K=17, ans_bytes=4 * 17 * 7 * 13), 'K = 17 slots'), (dict(LABELS, K=0), 'K = 0 slots'), (dict(LABELS, K=17), 'K = 17 slots'),
    (dict(ans=0), 'null address .answer 0,'), (dict(ids=0), r'null address .*ids 0\)'),
    (dict(ans_bytes=4 * 3 * 7 * 13 - 1), r'answer \(1092 bytes\) leaves its 1091-byte buffer'), (dict(LABELS, ans_bytes=90), r'answer \(91 bytes\) leaves its 90-byte buffer'),
    (dict(ans_bytes=-1), 'answer_bytes -1 is not a size'), (dict(ans_bytes=1 << 47), 'answer_bytes %d is not a size' % (1 << 47)),
    (dict(ans=ANS + 2), 'stack at 0x300002 is not 4-byte aligned'),
]


@pytest.mark.parametrize('change,message', REFUSED, ids=[m for _, m in REFUSED])
def test_bad_rows_are_refused_before_anything_is_enqueued(change, message):
    """The checks read the host table alone: nothing follows an address, so no device is needed to get FRTM_ERR_ARG -- and a launch
    through these addresses would not return at all."""
    rc, msg = _call([_row(), _row(**change)])
    assert rc == FRTM_ERR_ARG and ENTRY in msg and 'frame 1' in msg and re.search(message, msg), msg


def test_a_misaligned_label_map_is_fine_as_far_as_the_host_checks_go():
    """Only a stack needs 4-byte alignment: the same odd address as a label map passes every check up to the one that follows it."""
    rc, msg = _call([_row(**dict(LABELS, ans=ANS + 1))], out_words=16 * 12 - 1)
    assert rc == FRTM_ERR_ARG and 'out holds 191 words' in msg, msg


def test_bad_calls_are_refused_before_anything_is_enqueued():
    for kw, message in ((dict(n=0), 'n = 0'), (dict(n=-1), 'n = -1'), (dict(n=65536), 'n = 65536'), (dict(host=False), 'null table'), (dict(dev=False), 'null table'),
                        (dict(out=None), 'null out'), (dict(out_words=16 * 12 - 1), 'out holds 191 words, 1 frames need 192'), (dict(out_words=0), 'out holds 0 words')):
        rc, msg = _call([_row()], **kw)
        assert rc == FRTM_ERR_ARG and ENTRY in msg and message in msg, (kw, msg)
    rc, msg = _call([_row(), _row()], out_words=2 * 16 * 12 - 1)
    assert rc == FRTM_ERR_ARG and 'out holds 383 words, 2 frames need 384' in msg, msg


# ---- the reference against the loop ----------------------------------------------------------------------------------------------------
def test_numpy_reference_equals_the_loop_on_random_maps():
    rng = np.random.default_rng(7)
    for trial in range(6):
        ids = [[0, 3, 200], [5], [255, 0, 9, 77], [0, 1], [2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32], [9, 3]][trial]
        labels = O.blob_labels(rng, 5, 7, sorted(set(ids) | {41}))     # 41 is never listed
        assert np.array_equal(O.words(labels, ids), O.words_loop(labels, ids)), (trial, labels)
    placed_all = set()
    for K in (1, 2, 3, 16):
        stack, placed = O.hand_placed(O.merged_stack(rng, K, 5, 7))
        placed_all |= set(placed)
        lut = rng.permutation(256)[:K].astype(np.uint8)
        got, want = O.words(stack, lut), O.words_loop(stack, lut)
        assert np.array_equal(got, want), (K, np.argwhere(got != want)[:8].tolist())
        assert int(got[:K, O.AREA].sum()) == 35 and not got[K:].any()
    assert placed_all == {name for name, _, _ in O.HAND}


def test_reference_on_hand_placed_pixels():
    stack = np.zeros((3, 1, 8), dtype=np.float32)
    stack[1, 0, :6] = [0.5, 0.50001, 0.75, 1.5, -0.25, np.nan]
    stack[2, 0, 2] = 0.75                                              # two equal planes: the first wins
    stack[2, 0, 5] = 0.625                                             # a NaN never wins
    stack[:, 0, 6] = [0.9, 0.75, 0.8]                                  # the background plane is the largest
    stack[:, 0, 7] = np.nan                                            # NaNs only: the background, q = 0
    assert O.decode(stack)[0].tolist() == [0, 1, 1, 1, 0, 2, 0, 0]
    assert O.q(np.array([0.5, 1.5, -0.25, np.nan, 1.0, 0.1], dtype=np.float32)).tolist() == [128, 255, 0, 0, 255, 26]      # 127.5 rounds to even
    w = O.words(stack, [0, 5, 9])
    assert np.array_equal(w, O.words_loop(stack, [0, 5, 9]))
    # slot 0: pixels 0, 4, 6, 7 (7 has no neighbour of another label); conf = q(m_0) there = 0 + 0 + q(0.9) + 0; its mass: plane 0 over all pixels
    assert w[0].tolist() == [4, 0, 0, 7, 0, 17, 0, 3, 4, 230, 230, 0]
    assert w[1].tolist() == [3, 1, 0, 3, 0, 6, 0, 2, 3, 128 + 191 + 255, 128 + 128 + 191 + 255 + 191, 5]
    assert w[2].tolist() == [1, 5, 0, 5, 0, 5, 0, 1, 1, 159, 191 + 159 + 204, 9]
    labels = np.array([[1, 1, 0], [1, 2, 0], [7, 7, 0]], dtype=np.uint8)
    w = O.words(labels, [1, 2, 9])                                     # 0 and 7 are not listed: no slot, but other labels
    assert w[0].tolist() == [3, 0, 0, 1, 1, 1, 1, 2, 3, 0, 0, 1] and w[1].tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 2]
    assert w[2].tolist() == [0, 3, 3, -1, -1, 0, 0, 0, 0, 0, 0, 9] and not w[3:].any()
    assert np.array_equal(w, O.words_loop(labels, [1, 2, 9]))
    whole = np.full((4, 6), 3, dtype=np.uint8)
    assert O.words(whole, [3])[0].tolist() == [24, 0, 0, 5, 3, 60, 36, 0, 2 * 4 + 2 * 6 - 4, 0, 0, 3]


# ---- ObjectReport ---------------------------------------------------------------------------------------------------------------------
def test_object_report_host_logic():
    from frtm_vos_amd import ops
    stack = np.zeros((3, 4, 6), dtype=np.float32)
    stack[0] = 0.75
    stack[0, 1:3, 2:5], stack[1, 1:3, 2:5] = 0, 0.5 + np.arange(1, 7).reshape(2, 3) / 16.0
    stack[2, 3, 5] = 0.25                                               # plane 2 never wins: an empty object with a soft area
    labels = np.array([[4, 4, 0], [0, 0, 0]], dtype=np.uint8)
    words = torch.from_numpy(np.stack([O.words(stack, [0, 7, 200]), O.words(labels, [4, 9])]))
    rep = ops.ObjectReport(words, [3, 2], [True, False])
    assert len(rep) == 2 and rep.cpu() is rep.cpu() and rep.cpu() is words          # (a host tensor is its own copy)
    a = rep.objects(0)
    assert list(a) == [0, 7, 200] and all(isinstance(v, ops.ObjectStats) for v in a.values())
    q = O.q(stack[1, 1:3, 2:5])
    assert a[7] == ops.ObjectStats(area=6, box=(2, 1, 4, 2), centroid=(3.0, 1.5), edge=6, border=0, confidence=int(q.sum()) / (255.0 * 6),
                                   soft_area=int(q.sum()) / 255.0)
    assert a[0].area == 18 and a[0].box == (0, 0, 5, 3) and a[0].border == 16 and a[0].edge == 10 and a[0].confidence == 191 / 255.0
    assert a[200] == ops.ObjectStats(0, None, None, 0, 0, None, 64 / 255.0)
    b = rep.objects(1)
    assert b[4] == ops.ObjectStats(2, (0, 0, 1, 0), (0.5, 0.0), 2, 2, None, None) and b[9] == ops.ObjectStats(0, None, None, 0, 0, None, None)
    with pytest.raises(TypeError, match=r'\(n, 16, 12\) int64'):
        ops.ObjectReport(words.float(), [3, 2], [True, False])
    with pytest.raises(TypeError, match=r'\(n, 16, 12\) int64'):
        ops.ObjectReport(words[:, :, :11], [3, 2], [True, False])
    with pytest.raises(ValueError, match='2 frames, 1 slot counts'):
        ops.ObjectReport(words, [3], [True, False])
    with pytest.raises(ValueError, match='slot counts'):
        ops.ObjectReport(words, [3, 17], [True, False])


def test_describe_frames_refuses_before_any_launch():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from frtm_vos_amd import ops
    cpu = torch.zeros(4, 6, dtype=torch.uint8)
    with pytest.raises(ValueError, match='0 frames'):
        ops.describe_frames([])
    with pytest.raises(ValueError, match='1 answers, 2 luts'):
        ops.describe_frames([cpu], luts=[None, None])
    with pytest.raises(ValueError, match='1 answers, None luts, 2 ids'):
        ops.describe_frames([cpu], ids=[[1], [2]])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.describe_frames([cpu], ids=[[1, 2]])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.describe_frames([cpu], ids=[(0,)])
    for bad in (cpu.float(), torch.zeros(2, 4, 6, dtype=torch.float64), torch.zeros(1, 4, 6, dtype=torch.uint8), 'labels', None):
        with pytest.raises(TypeError, match='label map or a'):
            ops.describe_frames([bad], ids=[[1]])
    for bad in (None, 7, 'ab', [1.0], [True], [[1]]):
        with pytest.raises(TypeError, match=r'ids'):
            ops.describe_frames([cpu], ids=[bad])
    for bad, message in (([], 'lists 0 ids'), (list(range(17)), 'lists 17 ids'), ([256], '0 .. 255'), ([-1], '0 .. 255'), ([3, 4, 3], 'lists an id twice'),
                         (torch.tensor([5, 5]), 'lists an id twice')):
        with pytest.raises(ValueError, match=message):
            ops.describe_frames([cpu], ids=[bad])
    with pytest.raises(TypeError, match=r'needs ids\[0\]'):
        ops.describe_frames([cpu])
    with FakeTensorMode():
        labels = torch.empty(4, 6, dtype=torch.uint8, device='cuda')
        stack = torch.empty(2, 4, 6, device='cuda')
        lut = torch.empty(2, dtype=torch.uint8, device='cuda')
        stack17 = torch.empty(17, 4, 6, device='cuda')
        small = torch.empty(16 * 12 - 1, dtype=torch.int64, device='cuda')
    with pytest.raises(TypeError, match=r'needs luts\[0\]'):
        ops.describe_frames([stack])
    with pytest.raises(TypeError, match=r'needs luts\[0\]'):
        ops.describe_frames([stack], luts=[lut[:1]])
    with pytest.raises(TypeError, match=r'needs luts\[0\]'):
        ops.describe_frames([stack], luts=[torch.zeros(2, dtype=torch.uint8)])          # the LUT of a stack lives on the device
    with pytest.raises(ValueError, match='17 planes'):
        ops.describe_frames([stack17], luts=[lut])
    with pytest.raises(TypeError, match='must be contiguous'):
        ops.describe_frames([labels.t()], ids=[[1]])
    with pytest.raises(ValueError, match='out holds 191 words, 1 frames need 192'):
        ops.describe_frames([labels], ids=[[1]], out=small)
    with pytest.raises(TypeError, match='out is an ops.ObjectReport or an int64 tensor'):
        ops.describe_frames([labels], ids=[[1]], out=lut)
    with pytest.raises(RuntimeError, match='out is on cpu.*no CPU fallback'):
        ops.describe_frames([labels], ids=[[1]], out=torch.zeros(192, dtype=torch.int64))


def test_tracker_and_pool_have_the_surface():
    from frtm_vos_amd.model.stream_pool import StreamPool
    from frtm_vos_amd.model.tracker import Tracker
    assert list(inspect.signature(Tracker.describe).parameters) == ['self', 'out']
    assert list(inspect.signature(StreamPool.describe).parameters) == ['self', 'sids', 'out']
    state = types.SimpleNamespace(native_labels=None, current_masks=None, targets={}, _native_bufs={})      # a tracker before its first frame
    with pytest.raises(ValueError, match='nothing was tracked'):
        Tracker.describe_answer(state, None)
    state.current_masks = torch.zeros(2, 8, 6)
    with pytest.raises(ValueError, match='2 planes, the tracker 0 objects'):
        Tracker.describe_answer(state, None)
    state.targets = {5: None}
    state._object_lut = lambda: 'lut'
    stack, lut = Tracker.describe_answer(state, None)
    assert lut == 'lut' and stack.data_ptr() == state.current_masks.data_ptr()
    labels = torch.zeros(1, 16, 12, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r'no answer of size \(16, 12\) with 2 planes'):
        Tracker.describe_answer(state, labels)
    planes = torch.zeros(2 * 16 * 12)
    state._native_bufs[(1, 2, (16, 12), True)] = (None, planes)
    stack, _ = Tracker.describe_answer(state, labels)
    assert tuple(stack.shape) == (2, 16, 12) and stack.data_ptr() == planes.data_ptr()
    mine = torch.zeros(2, 16, 12)
    assert Tracker.describe_answer(state, labels, mine)[0] is mine


# ---- the kernel's budget ---------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_and_spill_nothing():
    assert os.path.exists(HIPCC), 'hipcc is needed (the build needs it as well)'
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'object_report.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'object_report.hip')], check=True, capture_output=True, cwd=d)
        isa = open(out).read()
    meta = isa[isa.index('amdhsa.kernels:'):]
    for kernel, lds in (('k_describe_frames', True), ('k_object_begin', False)):
        blocks = [b for b in meta.split('\n  - ') if re.search(r'\.name:\s+_Z%d%s[A-Z]' % (len(kernel), kernel), b)]
        assert len(blocks) == 1
        field = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, blocks[0]).group(1))
        print('%s: %d VGPRs, %d SGPRs, %d bytes of LDS' % (kernel, field('vgpr_count'), field('sgpr_count'), field('group_segment_fixed_size')))
        assert field('vgpr_spill_count') == 0 and field('sgpr_spill_count') == 0 and field('private_segment_fixed_size') == 0
        assert (0 < field('group_segment_fixed_size') <= 16 * 1024) if lds else field('group_segment_fixed_size') == 0      # four workgroups and more per CU
        assert not re.search(r'\.uses_dynamic_stack:\s+true', blocks[0])
