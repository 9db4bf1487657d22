"""The run-length coder without a GPU (csrc/mask_runs.hip, ops.encode_frames / MaskRuns): the ABI, the refusals of the C entries (they run
on the host, before anything is enqueued), the numpy statement of tests/_runs_refs.py against a plain loop over pixels, the worked examples of
include/frtm_hip.h, COCO's string form, MaskRuns' host logic, the wrapper's refusals and the kernels' scratch / spill / LDS budget.  The
kernels themselves are checked on the GPU (tests/test_mask_runs_gpu.py).  Everything is an integer: all comparisons are equalities."""
import ctypes
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _runs_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = '/opt/rocm/bin/hipcc'
ENTRY = 'frtm_encode_frames'
FRTM_ERR_ARG = -1


def test_abi_declares_exports_and_binds_the_entry_points():
    from frtm_vos_amd import _hip, build, ops
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'frtm_hip.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+%s\s*\(' % ENTRY, hdr) and hasattr(_hip.lib(), ENTRY)
    assert re.search(r'\bsize_t\s+frtm_encode_work_bytes\s*\(', hdr) and hasattr(_hip.lib(), 'frtm_encode_work_bytes')
    res, args = _hip.SIGNATURES[ENTRY]
    assert res is _hip.I and len(args) == 10                           # two tables, n, heads + words, runs + capacity, work + bytes, stream
    assert _hip.SIGNATURES['frtm_encode_work_bytes'] == (ctypes.c_size_t, [_hip.P, _hip.I, ctypes.c_size_t])
    assert 'mask_runs.hip' in build.SOURCES
    assert int(re.search(r'#define\s+FRTM_RUNS_HEAD_WORDS\s+(\d+)', hdr).group(1)) == ops.RUNS_HEAD_WORDS == R.HEAD == 4
    assert ops.OBJECT_SLOTS == R.SLOTS == 16
    # the row check exists once: both kernel files take it from the shared header
    for name in ('object_report.hip', 'mask_runs.hip'):
        src = open(os.path.join(ROOT, 'frtm-vos_amd', 'csrc', name)).read()
        assert '#include "object_rows.h"' in src and 'int ob_check(' not in src


# ---- the two restatements ---------------------------------------------------------------------------------------------------------------
def test_worked_examples_counts_and_strings():
    from frtm_vos_amd import ops
    m = np.array([[0, 1, 1, 0], [0, 1, 0, 0], [1, 1, 0, 1]], dtype=bool)
    assert R.counts(m) == R.counts_loop(m) == [2, 5, 4, 1]
    assert R.counts(np.zeros((1080, 1920), dtype=bool)) == [2073600] and R.counts(np.ones((1080, 1920), dtype=bool)) == [0, 2073600]
    assert R.counts_loop(np.zeros((3, 5), dtype=bool)) == [15] and R.counts_loop(np.ones((3, 5), dtype=bool)) == [0, 15]
    for c, s in (([2, 5, 4, 1], b'254L'), ([0, 2073600], b'0PPYo1'), ([5, 100000, 3, 2, 70000], b'5PeQ33R[nL][T2')):
        assert ops.rle_to_string(c) == R.to_string(c) == s
        assert ops.rle_from_string(s) == c and ops.rle_from_string(s.decode()) == c
    assert np.array_equal(ops.rle_decode((3, 4), [2, 5, 4, 1]), m) and np.array_equal(ops.rle_decode([3, 4], b'254L'), m)
    # a run continues from the bottom of a column into the top of the next: (h - 1, 1) and (0, 2) are one run of two
    m = np.zeros((4, 5), dtype=bool)
    m[3, 1], m[0, 2] = True, True
    assert R.counts(m) == R.counts_loop(m) == [7, 2, 11]
    with pytest.raises(ValueError, match='sum to 11'):
        ops.rle_decode((3, 4), [2, 5, 4])
    with pytest.raises(ValueError, match='ends inside a value'):
        ops.rle_from_string(b'25P')
    with pytest.raises(ValueError, match='no character of the code'):
        ops.rle_from_string(b'2 5')


def test_numpy_counts_equal_the_loop_on_random_and_hand_placed_masks():
    rng = np.random.default_rng(11)
    for trial in range(40):
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        m = rng.random((h, w)) < (0.1, 0.5, 0.9)[trial % 3]
        c = R.counts(m)
        assert c == R.counts_loop(m), (trial, m)
        assert sum(c) == h * w and sum(c[1::2]) == int(m.sum()) and all(v > 0 for v in c[1:])
        flat = m.flatten(order='F')
        assert len(c) == int((flat[1:] != flat[:-1]).sum()) + 1 + int(flat[0])
        assert np.array_equal(R.decode_counts((h, w), c), m)
    board = (np.add.outer(np.arange(5), np.arange(4)) % 2).astype(bool)   # odd height: the bit changes at every pixel, column ends included
    assert R.counts(board) == R.counts_loop(board) == [1] * 20
    board = (np.add.outer(np.arange(4), np.arange(3)) % 2).astype(bool)   # even height: a column ends on the bit the next starts with
    assert R.counts(board) == R.counts_loop(board) == [1, 1, 1, 2, 1, 1, 2, 1, 1, 1]


def test_slots_and_layout_of_the_reference():
    stack = np.zeros((3, 1, 8), dtype=np.float32)
    stack[1, 0, :6] = [0.5, 0.50001, 0.75, 1.5, -0.25, np.nan]
    stack[2, 0, 2] = 0.75                                              # two equal planes: the first wins
    stack[2, 0, 5] = 0.625                                             # a NaN never wins
    stack[:, 0, 6] = [0.9, 0.75, 0.8]                                  # the background plane is the largest
    stack[:, 0, 7] = np.nan                                            # NaNs only: the background
    assert R.slots(stack, [0, 5, 9])[0].tolist() == [0, 1, 1, 1, 0, 2, 0, 0]
    labels = np.array([[1, 1, 0], [1, 2, 0], [7, 7, 0]], dtype=np.uint8)
    assert R.slots(labels, [1, 2, 9]).tolist() == [[0, 0, -1], [0, 1, -1], [-1, -1, -1]]     # 0 and 7 are not listed: no slot
    heads, runs, needed = R.layout([stack, labels], [[0, 5, 9], [1, 2, 9]])
    assert heads[0, :3].tolist() == [[6, 0, 4, 0], [3, 6, 3, 5], [3, 9, 1, 9]] and not heads[0, 3:].any()
    assert heads[1, :3].tolist() == [[5, 12, 3, 1], [3, 17, 1, 2], [1, 20, 0, 9]] and not heads[1, 3:].any() and needed == 21
    assert runs.tolist() == [0, 1, 3, 1, 1, 2] + [1, 3, 4] + [5, 1, 2] + [0, 2, 1, 1, 5] + [4, 1, 4] + [9]
    cut_heads, cut, cut_needed = R.layout([stack, labels], [[0, 5, 9], [1, 2, 9]], capacity=5)
    assert cut.tolist() == [0, 1, 3, 1, 1] and np.array_equal(cut_heads, heads) and cut_needed == 21     # the heads hold the truth, overflow or not


def test_string_codec_and_decode_invert_on_200_random_masks():
    from frtm_vos_amd import ops
    rng = np.random.default_rng(12)
    negative = big = 0
    for trial in range(200):
        if trial % 10 == 0:
            h, w = 300, 400                                             # runs above 2^15 = 32768
            m = np.zeros((h, w), dtype=bool)
            m[:, 150:152 + trial % 7] = True
            m[int(rng.integers(0, h)), int(rng.integers(0, w))] ^= True
        else:
            h, w = int(rng.integers(1, 24)), int(rng.integers(1, 24))
            m = R.blob_labels(rng, h, w, [0, 1]).astype(bool) if trial % 2 else rng.random((h, w)) < 0.3
        c = R.counts(m)
        s = ops.rle_to_string(c)
        assert s == R.to_string(c) and ops.rle_from_string(s) == c
        assert np.array_equal(ops.rle_decode((h, w), c), m) and np.array_equal(ops.rle_decode((h, w), s), m)
        negative += any(c[i] < c[i - 2] for i in range(3, len(c)))
        big += max(c) > 2 ** 15
    assert negative >= 50 and big >= 20


# ---- refusals of the C entries: addresses that are never followed ------------------------------------------------------------------------
ANS, IDS, HEADS, RUNS, WORK = 0x300000, 0x400000, 0x500000, 0x600000, 0x700000
KEYS = ['form', 'h', 'w', 'ans', 'ans_bytes', 'K', 'ids', 'zero']


def _row(**kw):
    """A valid row: a 7 x 13 stack of K = 3 planes."""
    row = dict(form=1, h=7, w=13, ans=ANS, ans_bytes=4 * 3 * 7 * 13, K=3, ids=IDS, zero=0)
    row.update(kw)
    return [row[k] for k in KEYS]


def _table(rows):
    return (ctypes.c_longlong * (8 * len(rows)))(*[int(v) for r in rows for v in r])


def _work_bytes(rows, n=None, capacity=100):
    from frtm_vos_amd import _hip
    L = _hip.lib()
    t = _table(rows)
    got = L.frtm_encode_work_bytes(ctypes.addressof(t), len(rows) if n is None else n, capacity)
    return got, L.frtm_last_error().decode()


def _call(rows, n=None, host=True, dev=True, heads=HEADS, head_words=None, runs=RUNS, capacity=100, work=WORK, work_bytes=1 << 30):
    from frtm_vos_amd import _hip
    L = _hip.lib()
    t = _table(rows)
    n = len(rows) if n is None else n
    rc = L.frtm_encode_frames(ctypes.addressof(t) if host else None, ctypes.addressof(t) if dev else None, n, heads,
                              16 * 4 * max(n, 0) if head_words is None else head_words, runs, capacity, work, work_bytes, None)
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
    """Everything frtm_describe_frames refuses for its table, with the same words.  The checks read the host table alone: nothing follows an
    address, so no device is needed to get FRTM_ERR_ARG -- and a launch through these addresses would not return at all."""
    rows = [_row(), _row(**change)]
    rc, msg = _call(rows)
    assert rc == FRTM_ERR_ARG and ENTRY in msg and 'frame 1' in msg and re.search(message, msg), msg
    size, msg = _work_bytes(rows)
    assert size == 0 and 'frtm_encode_work_bytes' in msg and 'frame 1' in msg and re.search(message, msg), msg


def test_bad_calls_are_refused_before_anything_is_enqueued():
    need = _work_bytes([_row()])[0]
    assert need > 0
    for kw, message in ((dict(n=0), 'n = 0'), (dict(n=-1), 'n = -1'), (dict(n=65536), 'n = 65536'), (dict(host=False), 'null table'), (dict(dev=False), 'null table'),
                        (dict(heads=None), 'null heads, runs or work'), (dict(runs=None), 'null heads, runs or work'), (dict(work=None), 'null heads, runs or work'),
                        (dict(heads=HEADS + 4), '8-byte aligned'), (dict(runs=RUNS + 2), '8-byte aligned'), (dict(work=WORK + 4), '8-byte aligned'),
                        (dict(head_words=16 * 4 - 1), 'heads holds 63 words, 1 frames need 64'), (dict(head_words=0), 'heads holds 0 words'),
                        (dict(work_bytes=need - 1), 'work holds %d bytes, frtm_encode_work_bytes asks for %d' % (need - 1, need)), (dict(work_bytes=0), 'work holds 0 bytes'),
                        (dict(capacity=0), 'run_capacity = 0'), (dict(capacity=(1 << 40) + 1), 'run_capacity = %d' % ((1 << 40) + 1))):
        rc, msg = _call([_row()], **dict(dict(work_bytes=need), **kw))
        assert rc == FRTM_ERR_ARG and ENTRY in msg and message in msg, (kw, msg)
    rc, msg = _call([_row(), _row()], head_words=2 * 16 * 4 - 1)
    assert rc == FRTM_ERR_ARG and 'heads holds 127 words, 2 frames need 128' in msg, msg
    for kw, message in ((dict(n=0), 'n = 0'), (dict(n=65536), 'n = 65536'), (dict(capacity=0), 'run_capacity = 0'), (dict(capacity=(1 << 40) + 1), 'run_capacity')):
        size, msg = _work_bytes([_row()], **kw)
        assert size == 0 and 'frtm_encode_work_bytes' in msg and message in msg, (kw, msg)
    from frtm_vos_amd import _hip
    assert _hip.lib().frtm_encode_work_bytes(None, 1, 100) == 0 and 'null table' in _hip.lib().frtm_last_error().decode()
    assert _work_bytes([_row()], capacity=1 << 40)[0] == need           # the largest capacity is one


def test_work_bytes_is_monotone_in_n_and_in_the_sizes():
    def wb(h, w, K=3, n=1, stack=True):
        row = _row(h=h, w=w, K=K, ans_bytes=1 << 45) if stack else _row(form=0, h=h, w=w, K=K, ans_bytes=1 << 45)
        size, msg = _work_bytes([row] * n)
        assert size > 0, msg
        return size
    sizes = [1, 2, 63, 64, 65, 127, 128, 129, 1080, 1920, 16384]
    for a, b in zip(sizes, sizes[1:]):
        for other in (1, 64, 1080):
            assert wb(a, other) <= wb(b, other) and wb(other, a) < wb(other, b)
    assert wb(64, 64) < wb(65, 64) and wb(64, 64) < wb(64, 65)           # one more segment, one more column
    per_n = [wb(1080, 1920, n=n) for n in (1, 2, 5, 8)]
    assert per_n == sorted(set(per_n))
    assert wb(33, 70, K=1) < wb(33, 70, K=2) < wb(33, 70, K=16)
    assert wb(33, 70, K=3) == wb(33, 70, K=3, stack=False)               # the form does not enter
    # the size the header states: 4 (16 n + 2 n C), C = the most K w ceil(h / 64) of a frame
    assert wb(1080, 1920) == 4 * (16 + 2 * 3 * 1920 * 17)
    mixed, _ = _work_bytes([_row(h=10, w=10, K=1, ans_bytes=1 << 45), _row(h=1080, w=1920, ans_bytes=1 << 45)])
    assert mixed == 4 * (32 + 2 * 2 * 3 * 1920 * 17)
    assert wb(16384, 16384, K=16) == 4 * (16 + 2 * 16 * 16384 * 256)


# ---- MaskRuns -----------------------------------------------------------------------------------------------------------------------------
def _host_runs(answers, ids, capacity=None):
    from frtm_vos_amd import ops
    heads, runs, needed = R.layout(answers, ids)
    capacity = needed + 3 if capacity is None else capacity
    buf = torch.full((capacity + 2,), -7, dtype=torch.int32)
    buf[:min(needed, capacity)] = torch.from_numpy(runs[:capacity]).int()
    return ops.MaskRuns(torch.from_numpy(heads), buf, [a.shape[-2:] for a in answers], [len(i) for i in ids], capacity), needed


def test_mask_runs_host_logic():
    from frtm_vos_amd import ops
    labels = np.array([[4, 4, 0], [0, 9, 0]], dtype=np.uint8)
    other = np.array([[0, 1, 1, 0], [0, 1, 0, 0], [1, 1, 0, 1]], dtype=np.uint8)
    coded, needed = _host_runs([labels, other], [[4, 9], [1]])
    assert len(coded) == 2 and coded.cpu() is coded.cpu() and needed == 5 + 3 + 4
    assert coded.cpu()[1].tolist() == [0, 1, 1, 1, 3] + [3, 1, 2] + [2, 5, 4, 1]      # runs[:needed], not the whole buffer
    assert coded.counts(0) == {4: [0, 1, 1, 1, 3], 9: [3, 1, 2]} and coded.counts(1) == {1: [2, 5, 4, 1]}
    assert coded.rle(1) == {1: {'size': [3, 4], 'counts': [2, 5, 4, 1]}} and coded.rle(1, compressed=True) == {1: {'size': [3, 4], 'counts': b'254L'}}
    for oid, r in coded.rle(0).items():
        assert np.array_equal(ops.rle_decode(r['size'], r['counts']), labels == oid)
    short, needed = _host_runs([labels, other], [[4, 9], [1]], capacity=11)
    with pytest.raises(ops.RunsOverflow, match='need 12 elements and runs holds 11; call encode again with capacity=12') as e:
        short.cpu()
    assert isinstance(e.value, ValueError) and (e.value.needed, e.value.capacity) == (12, 11)
    with pytest.raises(ops.RunsOverflow):                                # every time, not only the first
        short.counts(0)
    heads = torch.zeros(1, 16, 4, dtype=torch.int64)
    runs = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(TypeError, match=r'\(n, 16, 4\) int64'):
        ops.MaskRuns(heads.int(), runs, [(2, 2)], [1], 8)
    with pytest.raises(TypeError, match=r'\(n, 16, 4\) int64'):
        ops.MaskRuns(heads[:, :, :3], runs, [(2, 2)], [1], 8)
    with pytest.raises(TypeError, match='1-d int32'):
        ops.MaskRuns(heads, runs.long(), [(2, 2)], [1], 8)
    with pytest.raises(ValueError, match='1 frames, 2 slot counts'):
        ops.MaskRuns(heads, runs, [(2, 2)], [1, 1], 8)
    with pytest.raises(ValueError, match='capacity 9 of a runs of 8'):
        ops.MaskRuns(heads, runs, [(2, 2)], [1], 9)
    assert ops.default_run_capacity([(1080, 1920), (7, 13)], [3, 2]) == 3 * (8 * 1920 + 8) + 2 * (8 * 13 + 8)


def test_encode_frames_refuses_before_any_launch():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from frtm_vos_amd import ops
    cpu = torch.zeros(4, 6, dtype=torch.uint8)
    with pytest.raises(ValueError, match='encode_frames: 0 frames'):
        ops.encode_frames([])
    with pytest.raises(ValueError, match='encode_frames: 1 answers, 2 luts'):
        ops.encode_frames([cpu], luts=[None, None])
    with pytest.raises(ValueError, match='1 answers, None luts, 2 ids'):
        ops.encode_frames([cpu], ids=[[1], [2]])
    with pytest.raises(RuntimeError, match='encode_frames: answer 0 is on cpu.*no CPU fallback'):
        ops.encode_frames([cpu], ids=[[1, 2]])
    for bad in (cpu.float(), torch.zeros(2, 4, 6, dtype=torch.float64), torch.zeros(1, 4, 6, dtype=torch.uint8), 'labels', None):
        with pytest.raises(TypeError, match='encode_frames: answer 0 is a .* label map or a'):
            ops.encode_frames([bad], ids=[[1]])
    for bad in (None, 7, 'ab', [1.0], [True], [[1]]):
        with pytest.raises(TypeError, match=r'encode_frames: .*ids'):
            ops.encode_frames([cpu], ids=[bad])
    for bad, message in (([], 'lists 0 ids'), (list(range(17)), 'lists 17 ids'), ([256], '0 .. 255'), ([-1], '0 .. 255'), ([3, 4, 3], 'lists an id twice')):
        with pytest.raises(ValueError, match=message):
            ops.encode_frames([cpu], ids=[bad])
    with FakeTensorMode():
        labels = torch.empty(4, 6, dtype=torch.uint8, device='cuda')
        stack = torch.empty(2, 4, 6, device='cuda')
        lut = torch.empty(2, dtype=torch.uint8, device='cuda')
        stack17 = torch.empty(17, 4, 6, device='cuda')
        heads = torch.empty(1, 16, 4, dtype=torch.int64, device='cuda')
        runs = torch.empty(50, dtype=torch.int32, device='cuda')
    with pytest.raises(TypeError, match=r'needs luts\[0\]'):
        ops.encode_frames([stack])
    with pytest.raises(TypeError, match=r'needs luts\[0\]'):
        ops.encode_frames([stack], luts=[torch.zeros(2, dtype=torch.uint8)])            # the LUT of a stack lives on the device
    with pytest.raises(ValueError, match='17 planes'):
        ops.encode_frames([stack17], luts=[lut])
    with pytest.raises(TypeError, match='must be contiguous'):
        ops.encode_frames([labels.t()], ids=[[1]])
    for bad in (0, -1, (1 << 40) + 1, 2.5, True, 'many'):
        with pytest.raises(ValueError, match='capacity is 1 .. 2\\^40'):
            ops.encode_frames([labels], ids=[[1]], capacity=bad)
    with pytest.raises(TypeError, match='out is an ops.MaskRuns'):
        ops.encode_frames([labels], ids=[[1]], out=runs)
    out = ops.MaskRuns(heads, runs, [(4, 6)], [1], 50)
    with pytest.raises(ValueError, match='out holds 64 head words, 2 frames need 128'):
        ops.encode_frames([labels, labels], ids=[[1], [2]], out=out)
    with pytest.raises(ValueError, match='capacity 51, out holds 50 elements'):
        ops.encode_frames([labels], ids=[[1]], out=out, capacity=51)
    host = ops.MaskRuns(torch.zeros(1, 16, 4, dtype=torch.int64), torch.zeros(50, dtype=torch.int32), [(4, 6)], [1], 50)
    with pytest.raises(RuntimeError, match='out is on cpu.*no CPU fallback'):
        ops.encode_frames([labels], ids=[[1]], out=host)


def test_describe_and_encode_share_the_checks_and_the_table_cache():
    from frtm_vos_amd import ops
    for fn in (ops.encode_frames, ops.describe_frames):
        src = inspect.getsource(fn)
        assert '_object_frames(' in src and '_object_table(' in src


def test_tracker_and_pool_have_the_surface():
    from frtm_vos_amd.model.stream_pool import StreamPool
    from frtm_vos_amd.model.tracker import Tracker
    assert list(inspect.signature(Tracker.encode).parameters) == ['self', 'out', 'capacity']
    assert list(inspect.signature(StreamPool.encode).parameters) == ['self', 'sids', 'out', 'capacity']
    assert 'describe_answer' in inspect.getsource(Tracker.encode)


# ---- the kernels' budget -----------------------------------------------------------------------------------------------------------------
def test_kernels_use_no_scratch_and_spill_nothing():
    assert os.path.exists(HIPCC), 'hipcc is needed (the build needs it as well)'
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'mask_runs.s')
        subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'frtm-vos_amd', 'csrc', 'mask_runs.hip')], check=True, capture_output=True, cwd=d)
        isa = open(out).read()
    meta = isa[isa.index('amdhsa.kernels:'):]
    blocks = [b for b in meta.split('\n  - ') if re.search(r'\.name:\s+_Z\d+k_runs_', b)]
    assert len(blocks) == 4                                              # the walk twice (count, emit) and the two scans
    for b in blocks:
        field = lambda key: int(re.search(r'\.%s:\s+(\d+)' % key, b).group(1))
        print('%s: %d VGPRs, %d SGPRs, %d bytes of LDS' % (re.search(r'\.name:\s+(\S+)', b).group(1), field('vgpr_count'), field('sgpr_count'),
                                                           field('group_segment_fixed_size')))
        assert field('vgpr_spill_count') == 0 and field('sgpr_spill_count') == 0 and field('private_segment_fixed_size') == 0
        assert 0 < field('group_segment_fixed_size') <= 40 * 1024           # four workgroups per CU
        assert not re.search(r'\.uses_dynamic_stack:\s+true', b)
    assert 'global_atomic' not in isa and 'flat_atomic' not in isa          # no position depends on an order of arrival
