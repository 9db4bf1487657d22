"""The working-size option on the GPU: the two kernels of csrc/native_size.hip against the fp64 definition of tests/_native_refs.py, and
the plumbing through Tracker and StreamPool.

Kernel tolerances (tests/_native_refs.py): soft planes within SOFT_TOL = 2^-21 of the fp64 sum over the fp32 taps (at most six fp32
roundings on values in [0, 1]); labels equal to the fp64 decode except where its margin min(top - second, |top - 0.5|) is within
LABEL_MARGIN = 2^-20, and that band holds at most 1 % of a case's pixels.  On equal sizes: bit-identical to frtm_track_merge.

Plumbing: the plain tracker is bitwise reproducible from run to run (tests/test_stream_pool_gpu.py::test_two_pool_runs_are_bitwise_equal
relies on the same), so it adds no tolerance of its own: under the option a tracker fed native frames equals the plain tracker fed the
frames resized by hand, up to the kernel tolerances above."""
import pytest
import torch
import torch.nn.functional as F

import _native_refs as R

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = 'cuda'
POISON_U8, POISON_F32 = 0xAB, -7.0


def _lut(K, seed):
    """K distinct ids, lut[0] not 0: a label that ignores the LUT does not pass."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randperm(250, generator=g)[:K] + 3).to(torch.uint8)


def _check_frame(name, m, native, lut, labels, soft):
    """One frame of a launch against the definition: m (K,h,w) fp32 host, labels (H,W) uint8 and soft (K,H,W) (or None) from the device."""
    ref = R.native_planes(m, native)
    lab, margin = R.decode(ref)
    want = lut.long()[lab]
    excluded = margin <= R.LABEL_MARGIN
    wrong = (labels.cpu().long() != want) & ~excluded
    err = float((soft.cpu().double() - ref).abs().max()) if soft is not None else 0.0
    print('%s: max |soft - fp64| %.3e (bound %.3e), excluded share %.5f, labels wrong outside the band %d, label planes %r'
          % (name, err, R.SOFT_TOL, float(excluded.float().mean()), int(wrong.sum()), lab.unique().tolist()))
    assert err <= R.SOFT_TOL
    assert float(excluded.float().mean()) <= R.EXCLUDED_CAP
    assert int(wrong.sum()) == 0


@pytest.mark.parametrize('planes,size,native', R.SHAPES)
@pytest.mark.parametrize('with_soft', [True, False])
def test_masks_to_native_against_fp64(planes, size, native, with_soft):
    from frtm_vos_amd import ops
    m = R.merged(planes, size[0], size[1], planes * 100 + size[0])
    lut = _lut(planes, planes)
    table = ops.NativeTable.packed(size, [(planes,) + native], DEV, soft=with_soft)
    labels = torch.full((table.label_bytes + 64,), POISON_U8, dtype=torch.uint8, device=DEV)
    soft = torch.full((table.soft_elems + 64,), POISON_F32, device=DEV) if with_soft else None
    ops.masks_to_native(m.to(DEV), table, labels, lut.to(DEV), soft=soft)
    torch.cuda.synchronize()
    _check_frame('%r %r -> %r' % (planes, size, native), m, native, lut, table.labels_of(labels, 0), table.soft_of(soft, 0) if with_soft else None)
    assert bool((labels[table.label_bytes:] == POISON_U8).all())                         # nothing behind the frame's outputs
    if with_soft:
        assert bool((soft[table.soft_elems:] == POISON_F32).all())
        if size == native:
            assert torch.equal(table.soft_of(soft, 0).cpu(), m)


def test_one_packed_launch_with_different_plane_counts_and_a_row_that_names_no_frame():
    """Frames of one launch share the working size, so the three frames here are native sizes and plane counts of the shapes at the
    working size (40, 300): 16 planes -> (23, 31) (under half the working size: every tile walks 2 row chunks x 3 column chunks of its
    source footprint), 3 planes -> (90, 700) (enlarging, several tiles), 2 planes -> (40, 300) (the identity).  Mask offsets are odd
    numbers of floats (no 16-byte alignment), outputs are packed in another order than the rows, and one row's masks lie outside the
    buffer: the kernel skips it, and the outputs it names keep their poison."""
    from frtm_vos_amd import ops
    h, w = 40, 300
    frames = [(16, (23, 31)), (3, (90, 700)), (2, (40, 300))]
    ms = [R.merged(K, h, w, 7 + K) for K, _ in frames]
    luts = [_lut(K, 40 + K) for K, _ in frames]
    gaps = (3, 2, 2)                                                                      # -> offsets 3, 192005, 228007 floats
    buf, moffs = [], []
    for m, gap in zip(ms, gaps):
        buf.append(torch.full((gap,), 123.0))
        moffs.append(sum(t.numel() for t in buf))
        buf.append(m.reshape(-1))
    masks = torch.cat(buf)
    assert all(o % 4 != 0 for o in moffs)
    # outputs: frame 2 first, then the skipped row's region, then frame 0, then frame 1
    rows, lo, so, to, where = [None] * 4, 0, 0, 0, {}
    for r in (2, 3, 0, 1):
        K, (Hn, Wn) = frames[r] if r < 3 else (4, (6, 10))
        moff = moffs[r] if r < 3 else masks.numel() - 4 * h * w + 1                       # (row 3: its last plane leaves the mask buffer by one float)
        rows[r] = (moff, K, Hn, Wn, lo, so, to)
        where[r] = (lo, Hn * Wn, so, K * Hn * Wn)
        lo, so, to = lo + Hn * Wn, so + K * Hn * Wn, to + K
    table = ops.NativeTable(rows, DEV)
    lut_buf = torch.zeros(to, dtype=torch.uint8)
    for r in range(3):
        lut_buf[rows[r][6]:rows[r][6] + frames[r][0]] = luts[r]
    labels = torch.full((lo,), POISON_U8, dtype=torch.uint8, device=DEV)
    soft = torch.full((so,), POISON_F32, device=DEV)
    ops.masks_to_native(masks.to(DEV), table, labels, lut_buf.to(DEV), soft=soft, size=(h, w))
    torch.cuda.synchronize()
    for r in range(3):
        _check_frame('packed row %d' % r, ms[r], frames[r][1], luts[r], table.labels_of(labels, r), table.soft_of(soft, r))
    a, n, b, k = where[3]
    assert bool((labels[a:a + n] == POISON_U8).all()) and bool((soft[b:b + k] == POISON_F32).all())
    assert torch.equal(table.soft_of(soft, 2).cpu(), ms[2])                                # the identity row: bit for bit
    # a frame's result does not depend on what else the launch holds
    alone = ops.NativeTable.packed((h, w), [(16, 23, 31)], DEV)                           # (the chunked row)
    l1 = torch.empty(alone.label_bytes, dtype=torch.uint8, device=DEV)
    s1 = torch.empty(alone.soft_elems, device=DEV)
    ops.masks_to_native(ms[0].to(DEV), alone, l1, luts[0].to(DEV), soft=s1)
    assert torch.equal(alone.labels_of(l1, 0), table.labels_of(labels, 0)) and torch.equal(alone.soft_of(s1, 0), table.soft_of(soft, 0))


@pytest.mark.parametrize('n_obj,size', [(3, (6, 10)), (1, (6, 10)), (2, (37, 70))])
def test_on_equal_sizes_labels_and_planes_are_track_merges(n_obj, size):
    """frtm_track_merge on refiner logits gives merged masks and decoded labels; masks_to_native on those masks at the same size gives
    the same planes and the same labels, bit for bit (one object: track_merge's single-object branch)."""
    from frtm_vos_amd import ops
    frames = 2
    g = torch.Generator().manual_seed(n_obj)
    logits = (torch.randn(frames * n_obj, 1, *size, generator=g) * 3).to(DEV)
    logits.view(-1)[::7] = 0.0                                                            # sigmoid = 0.5 exactly: the tie of the decode
    lut = _lut(n_obj + 1, 5).to(DEV)
    masks = torch.empty(frames, n_obj + 1, *size, device=DEV)
    want = torch.empty(frames, 1, *size, dtype=torch.uint8, device=DEV)
    ops.track_merge(logits, frames, n_obj, masks, want, lut, single_object=n_obj == 1)
    table = ops.NativeTable.packed(size, [(n_obj + 1,) + size] * frames, DEV, shared_lut=True)
    labels = torch.empty(table.label_bytes, dtype=torch.uint8, device=DEV)
    soft = torch.empty(table.soft_elems, device=DEV)
    ops.masks_to_native(masks, table, labels, lut, soft=soft)
    torch.cuda.synchronize()
    assert torch.equal(labels.view_as(want), want) and torch.equal(soft.view_as(masks), masks)
    assert len(want.unique()) >= 2


@pytest.mark.parametrize('src,dst', [((37, 53), (12, 20)), ((5, 3), (11, 9))])
def test_resize_label_map_is_interpolate_nearest(src, dst):
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(src[0])
    maps = [torch.tensor([0, 1, 2, 255], dtype=torch.uint8)[torch.randint(0, 4, src, generator=g)] for _ in range(2)]
    pad = 5                                                                               # the second map starts at an odd byte offset
    flat = torch.cat([maps[0].reshape(-1), torch.zeros(pad, dtype=torch.uint8), maps[1].reshape(-1)])
    desc = torch.tensor([[0, src[0], src[1], 0], [maps[0].numel() + pad, src[0], src[1], 0]])
    got = ops.resize_label_map_u8(flat.to(DEV), desc, dst)
    again = ops.ResizePlan(desc, DEV).label_map(flat.to(DEV), dst)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2, 1) + dst and torch.equal(got, again)
    for k in range(2):
        want = F.interpolate(maps[k][None, None].float(), dst, mode='nearest')[0, 0].to(torch.uint8)
        assert torch.equal(got[k, 0].cpu(), want), k
        assert sorted(want.unique().tolist()) == [0, 1, 2, 255] or min(dst) > min(src)
    with pytest.raises(TypeError):
        ops.resize_label_map_u8(flat.float().to(DEV), desc, dst)


def test_resize_plan_gives_the_resize_functions_results():
    """ops.ResizePlan keeps the uploaded table; its launches are those of resize_frames_u8 / resize_labels_u8, into the caller's buffer."""
    from frtm_vos_amd import ops
    g = torch.Generator().manual_seed(3)
    frames = [torch.randint(0, 256, (3, 21, 34), generator=g, dtype=torch.uint8), torch.randint(0, 256, (3, 40, 17), generator=g, dtype=torch.uint8)]
    flat = torch.cat([f.reshape(-1) for f in frames]).to(DEV)
    desc = torch.tensor([[0, 21, 34, 0], [frames[0].numel(), 40, 17, 0]])
    want = ops.resize_frames_u8(flat, desc, 3, (16, 24))
    plan = ops.ResizePlan(desc, DEV)
    out = torch.zeros(2, 3, 16, 24, dtype=torch.uint8, device=DEV)
    assert plan.frames(flat, 3, (16, 24), out=out) is out
    assert torch.equal(out, want) and torch.equal(plan.frames(flat, 3, (16, 24)), want)
    ldesc = torch.tensor([[0, 21, 34, 7], [21 * 34, 21, 34, 9]])
    assert torch.equal(ops.ResizePlan(ldesc, DEV).labels(flat, (16, 24)), ops.resize_labels_u8(flat, ldesc, (16, 24)))
    with pytest.raises(TypeError):
        plan.frames(flat, 3, (16, 24), out=out[:1])


# ----------------------------------------------------------------------------------------------------------------------------------
# Tracker
# ----------------------------------------------------------------------------------------------------------------------------------
WS = (128, 160)
BIG = (256, 320)


def _score_following(chans):
    from frtm_vos_amd.lib.synthetic import make_score_following_refiner
    from frtm_vos_amd.model.seg_network import SegNetwork
    torch.manual_seed(1)
    return make_score_following_refiner(SegNetwork(1, 64, chans, True).eval())


def _params(working_size=None, following=False):
    """The configuration of tests/test_stream_pool_gpu.py.  ``following``: the synthetic stand-in for a trained refiner (masks confident
    where the target model scores, so label maps carry objects); else the seeded default refiner, whose masks stay below 0.5."""
    from frtm_vos_amd.evaluate import Parameters
    torch.manual_seed(0)
    kw = {} if working_size is None else dict(working_size=working_size)
    params = Parameters(None, fast=True, device=DEV, feature_extractor='resnet18', feature_batch=8, trunk_lanes=2, **kw)
    if following:
        params.refiner_factory = _score_following
    params.disc_params.update(memory_size=8, init_iters=(2, 3), update_iters=(3,))
    return params


def _seq(name, frames, size, n_obj, seed, late=None):
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    s = SyntheticSequence(name, frames, size, n_obj, seed=seed, late_object_at=late)
    s.preload(DEV)
    return s


def _literal_loop(trk, frames):
    """initialize(), then track(image) frame by frame on ``frames`` = (image, labels, new_objects) -> ({frame: masks}, {frame: labels})."""
    trk.eval()
    soft, labels = {}, {}
    for i, (image, lb, new_objects) in enumerate(frames):
        had = len(trk.targets) > 0
        if len(new_objects) > 0:
            torch.manual_seed(0)
            trk.initialize(image.to(DEV), lb.to(DEV), new_objects)
        if had:
            soft[i] = trk.track(image.to(DEV)).clone()
            labels[i] = None if trk.native_labels is None else trk.native_labels.clone()
        trk.current_frame += 1
    torch.cuda.synchronize()
    return soft, labels


def _resized_by_hand(seq, size):
    """The sequence's frames through ops.resize_frames_u8 ('area') and its label maps through ops.resize_label_map_u8."""
    from frtm_vos_amd import ops
    out = []
    for image, lb, new_objects in seq:
        Hn, Wn = image.shape[-2:]
        im = ops.resize_frames_u8(image.contiguous().view(-1), torch.tensor([[0, Hn, Wn, ops.RESIZE_MODES['area']]]), 3, size)[0]
        if len(new_objects) > 0:
            lb = ops.resize_label_map_u8(lb.contiguous().view(-1), torch.tensor([[0, Hn, Wn, 0]]), size)[0]
        out.append((im, lb, new_objects))
    return out


def _compare_with_upsampled(name, got_soft, got_labels, ref_soft, native, ids, objects):
    """got: the option's native-size answers; ref_soft: the plain tracker's working-size masks of the same frames.  The reference is those
    masks upsampled: by torch's bilinear on the device (fp32) and by the fp64 definition, both within SOFT_TOL of the kernel; labels by the
    rule, equal outside the margin band."""
    assert sorted(got_soft) == sorted(ref_soft) and len(ref_soft) >= 5
    lut = torch.tensor([0] + list(ids))
    for t in sorted(ref_soft):
        m = ref_soft[t]
        assert tuple(got_soft[t].shape) == (m.shape[0],) + native and tuple(got_labels[t].shape) == (1,) + native
        up = F.interpolate(m[None], native, mode='bilinear', align_corners=False)[0]
        ref = R.native_planes(m.cpu(), native)
        e_t, e_d = float((got_soft[t] - up).abs().max()), float((got_soft[t].cpu().double() - ref).abs().max())
        lab, margin = R.decode(ref)
        excluded = margin <= R.LABEL_MARGIN
        wrong = (got_labels[t][0].cpu().long() != lut[lab]) & ~excluded
        print('%s frame %d: max |soft - torch| %.3e, |soft - fp64| %.3e, excluded share %.5f, wrong labels %d, object pixels %d'
              % (name, t, e_t, e_d, float(excluded.float().mean()), int(wrong.sum()), int((lab > 0).sum())))
        assert e_t <= R.SOFT_TOL and e_d <= R.SOFT_TOL
        assert float(excluded.float().mean()) <= R.EXCLUDED_CAP and int(wrong.sum()) == 0
    spread = float(torch.cat([ref_soft[t][1:].reshape(-1) for t in ref_soft]).std())
    pixels = sum(int((R.decode(ref_soft[t].cpu().double())[0] > 0).sum()) for t in ref_soft)
    print('%s: spread of the object planes %.2e, object pixels at the working size %d' % (name, spread, pixels))
    assert spread > 1e-3 and (pixels > 0 or not objects)             # the masks are not trivial; with the stand-in refiner the labels carry objects


def test_frames_at_the_working_size_take_the_plain_path_bit_for_bit():
    """(i) working_size = the frames' size: masks of the literal loop and labels of run_sequence equal the plain tracker's, bit for bit."""
    seq = _seq('same', 7, WS, 2, 21)
    plain, _ = _literal_loop(_params().get_model(), seq)
    trk = _params(WS).get_model()
    assert trk.working_size == WS
    opt, opt_labels = _literal_loop(trk, seq)
    assert sorted(plain) == sorted(opt) == list(range(1, 7)) and all(v is None for v in opt_labels.values())
    for t in plain:
        assert torch.equal(plain[t], opt[t]), t
    a, _ = _params().get_model().run_sequence(seq)                    # (_params seeds the generator: both draw the same target models)
    b, _ = _params(WS).get_model().run_sequence(seq)
    assert len(a) == len(b) == 7 and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.fixture(scope='module')
def big_sequence():
    return _seq('big', 7, BIG, 2, 22)


@pytest.fixture(scope='module')
def big_loop(big_sequence):
    return _literal_loop(_params(WS).get_model(), big_sequence)


@pytest.mark.parametrize('following', [False, True])
def test_native_frames_equal_the_plain_tracker_on_frames_resized_by_hand(big_sequence, big_loop, following):
    """(ii) six 256 x 320 frames at working size 128 x 160."""
    got = _literal_loop(_params(WS, following).get_model(), big_sequence) if following else big_loop
    ref, _ = _literal_loop(_params(None, following).get_model(), _resized_by_hand(big_sequence, WS))
    assert all(tuple(m.shape[-2:]) == WS for m in ref.values())
    _compare_with_upsampled('track()', got[0], got[1], ref, BIG, big_sequence.obj_ids, following)


def test_state_stays_at_the_working_size(big_sequence):
    trk = _params(WS).get_model().eval()
    image, lb, new = big_sequence[0]
    torch.manual_seed(0)
    masks = trk.initialize(image, lb, new)
    assert tuple(masks.shape) == (3,) + WS and tuple(trk.current_masks.shape) == (3,) + WS
    trk.current_frame += 1
    out = trk.track(big_sequence[1][0])
    assert tuple(out.shape) == (3,) + BIG and tuple(trk.current_masks.shape) == (3,) + WS and tuple(trk.native_labels.shape) == (1,) + BIG
    again = trk.track(big_sequence[1][0][None])                       # a (1,3,H,W) frame: resized as such, the same answer
    assert tuple(again.shape) == (3,) + BIG and tuple(trk.current_masks.shape) == (3,) + WS
    small = trk._resize_in(big_sequence[2][0][None])[0]
    same = trk.track(small)                                            # a frame at the working size: the plain path, no stale label map
    assert same is trk.current_masks and trk.native_labels is None
    with pytest.raises(ValueError, match='ytvos_merge'):
        trk.run_sequence(big_sequence, ytvos_merge=True)
    with pytest.raises(TypeError):
        trk.track(big_sequence[1][0].float())


@pytest.mark.parametrize('following', [False, True])
def test_run_sequence_equals_the_literal_loop_under_the_option(big_sequence, big_loop, following):
    """(iii) run_sequence resizes whole trunk batches and decodes whole windows; the literal loop goes frame by frame.  The trunk sums in
    another order in a batch (tests/test_fullsize_gpu.py::test_run_sequence_matches_the_literal_per_frame_loop: agreement > 0.995)."""
    loop = _literal_loop(_params(WS, True).get_model(), big_sequence) if following else big_loop
    trk = _params(WS, following).get_model()
    torch.manual_seed(0)                                              # the first target model's draw, as in the loop
    outputs, _ = trk.run_sequence(big_sequence)
    assert len(outputs) == 7 and all(tuple(o.shape) == (1,) + BIG and o.dtype == torch.uint8 for o in outputs)
    assert torch.equal(outputs[0], big_sequence[0][1])
    agree = [float((outputs[t] == loop[1][t]).float().mean()) for t in range(1, 7)]
    print('run_sequence vs literal loop under working_size: label agreement per frame', ['%.5f' % a for a in agree],
          'object pixels on frame 6: %d' % int((outputs[6] > 0).sum()))
    assert min(agree) > 0.995, agree
    assert int((outputs[6] > 0).sum()) > 0 or not following


def test_a_late_object_under_the_option():
    """(iv) an object that appears on frame 3 goes through initialize() on that frame, at native size, in both loops."""
    seq = _seq('late', 7, BIG, 2, 23, late=3)
    soft, labels = _literal_loop(_params(WS, True).get_model(), seq)
    ref, _ = _literal_loop(_params(None, True).get_model(), _resized_by_hand(seq, WS))
    assert [soft[t].shape[0] for t in sorted(soft)] == [2, 2, 3, 3, 3, 3]
    _compare_with_upsampled('late object', soft, labels, ref, BIG, seq.obj_ids, True)
    trk = _params(WS, True).get_model()
    torch.manual_seed(0)
    outputs, _ = trk.run_sequence(seq)
    agree = [float((outputs[t] == labels[t]).float().mean()) for t in range(1, 7)]
    print('late object, run_sequence vs literal loop: label agreement per frame', ['%.5f' % a for a in agree],
          'pixels of the late object on frame 3: %d' % int((outputs[3] == 2).sum()))
    assert min(agree) > 0.995 and int((outputs[3] == 2).sum()) > 0      # (frame 3 carries the late object's start mask)


# ----------------------------------------------------------------------------------------------------------------------------------
# StreamPool
# ----------------------------------------------------------------------------------------------------------------------------------
POOL_SIZES = [(128, 160), (256, 320), (120, 200)]
POOL_OBJECTS = [1, 2, 2]
POOL_SOFT_TOL = 1.3e-4            # pool against loop: max over frames of mean |soft mask difference|


@pytest.fixture(scope='module')
def pool_sequences():
    return [_seq('p%d' % k, 6, size, n, 30 + k) for k, (size, n) in enumerate(zip(POOL_SIZES, POOL_OBJECTS))]


def _pool_run(seqs, working_size, ragged):
    pool = _params().get_stream_pool(max_streams=3, ragged_groups=ragged, working_size=working_size)
    sids = [pool.open() for _ in seqs]
    soft, labels, passes = [dict() for _ in seqs], [dict() for _ in seqs], []
    for t in range(len(seqs[0])):
        frames = {}
        for k, seq in enumerate(seqs):
            image, lb, new_objects = seq[t]
            if len(new_objects) > 0:
                torch.manual_seed(0)
                pool.initialize(sids[k], image, lb, new_objects)
            frames[sids[k]] = image
        before = pool.trunk_passes
        out = pool.step(frames)
        if out:
            passes.append(pool.trunk_passes - before)
        for k in range(len(seqs)):
            if sids[k] in out:
                soft[k][t] = out[sids[k]].clone()
                if sids[k] in pool.native_labels:
                    labels[k][t] = pool.native_labels[sids[k]].clone()
    torch.cuda.synchronize()
    for sid in sids:
        pool.close(sid)
    return soft, labels, passes


@pytest.fixture(scope='module')
def option_loops(pool_sequences):
    return [_literal_loop(_params(WS).get_model(), s) for s in pool_sequences]


@pytest.mark.parametrize('ragged', [False, True])
def test_pool_tracks_three_native_sizes_in_one_trunk_pass(pool_sequences, option_loops, ragged):
    soft, labels, passes = _pool_run(pool_sequences, WS, ragged)
    assert passes == [1] * 5                                           # one trunk pass per tick for the three sizes
    for k, (size, n) in enumerate(zip(POOL_SIZES, POOL_OBJECTS)):
        ref = option_loops[k][0]
        assert sorted(soft[k]) == sorted(ref) == list(range(1, 6))
        d_mean = max(float((soft[k][t] - ref[t]).abs().mean()) for t in ref)
        d_max = max(float((soft[k][t] - ref[t]).abs().max()) for t in ref)
        wrong = total = excluded = 0
        for t in ref:
            assert tuple(soft[k][t].shape) == (n + 1,) + size
            lab, margin = R.decode(ref[t].cpu().double())
            band = margin <= 2 * POOL_SOFT_TOL
            got = R.decode(soft[k][t].cpu().double())[0]
            wrong += int(((got != lab) & ~band).sum())
            excluded += int(band.sum())
            total += lab.numel()
            if size != WS:                                              # the kernel's own labels (object ids = plane indices here), decoded from what it wrote
                assert torch.equal(labels[k][t].cpu().long(), got), (k, t)
            else:
                assert t not in labels[k]                               # (its answer is current_masks: no way back, no map)
        print('stream %d %r ragged %r: max mean |soft diff| %.2e, max |soft diff| %.2e, labels wrong outside the band %d of %d (band %d)'
              % (k, size, ragged, d_mean, d_max, wrong, total, excluded))
        assert d_mean <= POOL_SOFT_TOL, (k, d_mean)
        assert wrong == 0 and excluded <= 0.01 * total, (k, wrong, excluded)


def test_without_the_option_three_sizes_make_three_passes_and_the_plain_results(pool_sequences):
    """Each stream is alone in its trunk pass and its group: the plain literal loop's masks, bit for bit
    (tests/test_stream_pool_gpu.py::test_a_pool_of_one_stream_is_bitwise_the_literal_loop)."""
    soft, labels, passes = _pool_run(pool_sequences, None, False)
    assert passes == [3] * 5 and all(not d for d in labels)
    for k, seq in enumerate(pool_sequences):
        ref, _ = _literal_loop(_params().get_model(), seq)
        assert sorted(soft[k]) == sorted(ref)
        for t in ref:
            assert torch.equal(soft[k][t], ref[t]), (k, t)


class _Frames:
    """A sequence over given (image, labels, new_objects) triples, with what run_sequence asks of one."""

    def __init__(self, name, obj_ids, frames):
        self.name, self.obj_ids, self.frames = name, list(obj_ids), list(frames)
        self.frame_names = ['%05d' % i for i in range(len(self.frames))]

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i]

    def __iter__(self):
        return iter(self.frames)


@pytest.mark.parametrize('late', [None, 3])
def test_run_sequence_equals_the_plain_run_sequence_on_frames_resized_by_hand(late):
    """(iii), sharper: both sides run the SAME trunk batches and windows at the working size (a frame's resize does not depend on the batch
    it is resized in), so the plain tracker's window masks are the option's state, and the option's label maps must be the rule's decode
    of those masks upsampled -- which isolates the batched resize and the window decode.  Stand-in refiner: the maps carry objects."""
    seq = _seq('rs', 7, BIG, 2, 24, late=late)
    trk = _params(WS, True).get_model()
    torch.manual_seed(0)
    outputs, _ = trk.run_sequence(seq)
    plain = _params(None, True).get_model()
    soft, tw = [], plain.track_window
    plain.track_window = lambda images, taps: (lambda m: (soft.extend(m.clone().unbind(0)), m)[1])(tw(images, taps))
    torch.manual_seed(0)
    small, _ = plain.run_sequence(_Frames('rs', seq.obj_ids, _resized_by_hand(seq, WS)))
    assert len(outputs) == len(small) == 7 and len(soft) == 6
    lut = torch.tensor([0] + list(seq.obj_ids))
    pixels = 0
    for t in range(1, 7):
        ref = R.native_planes(soft[t - 1].cpu(), BIG)
        lab, margin = R.decode(ref)
        excluded = margin <= R.LABEL_MARGIN
        wrong = (outputs[t][0].cpu().long() != lut[lab]) & ~excluded
        pixels += int((lab > 0).sum())
        print('run_sequence frame %d (late %r): excluded share %.5f, wrong labels %d, object pixels %d' % (t, late, float(excluded.float().mean()), int(wrong.sum()), int((lab > 0).sum())))
        assert tuple(outputs[t].shape) == (1,) + BIG and float(excluded.float().mean()) <= R.EXCLUDED_CAP and int(wrong.sum()) == 0
    assert pixels > 0


@pytest.mark.parametrize('ragged', [False, True])
def test_pool_way_back_with_objects_and_a_fallback(ragged):
    """The pool's way back on masks that carry objects (stand-in refiner), with a late object on a stream whose frames are NOT at the
    working size: on frame 3 that stream falls back to its own track() and its own way back.  Every native-size answer is held to the
    pool's own working-size state of that stream (tracker(sid).current_masks) upsampled by the fp64 definition: planes within SOFT_TOL,
    label maps = object ids by the rule outside the margin band.  A wrong LUT offset, plane offset or decode in the group launch fails here
    whatever the trunk's summation order does to the masks themselves."""
    sizes, objects, lates = [(128, 160), (256, 320), (120, 200)], [1, 3, 2], [None, 3, None]
    seqs = [_seq('w%d' % k, 6, s, n, 50 + k, late=l) for k, (s, n, l) in enumerate(zip(sizes, objects, lates))]
    params = _params(None, True)
    pool = params.get_stream_pool(max_streams=3, ragged_groups=ragged, working_size=WS)
    sids = [pool.open() for _ in seqs]
    fallbacks, pixels = 0, [0, 0, 0]
    for t in range(6):
        frames = {}
        for k, seq in enumerate(seqs):
            image, lb, new_objects = seq[t]
            if len(new_objects) > 0:
                torch.manual_seed(0)
                pool.initialize(sids[k], image, lb, new_objects)
            frames[sids[k]] = image
        eligible = {sid: pool._eligible(pool.tracker(sid), pool.tracker(sid).active_targets()) for sid in sids}
        out = pool.step(frames)
        torch.cuda.synchronize()
        for k, sid in enumerate(sids):
            if sid not in out:
                continue
            state = pool.tracker(sid).current_masks
            K = state.shape[0]
            assert tuple(state.shape[-2:]) == WS and tuple(out[sid].shape) == (K,) + sizes[k]
            if sizes[k] == WS:
                assert sid not in pool.native_labels and torch.equal(out[sid], state)
                continue
            fallbacks += 0 if eligible[sid] else 1
            ref = R.native_planes(state.cpu(), sizes[k])
            lab, margin = R.decode(ref)
            excluded = margin <= R.LABEL_MARGIN
            ids = torch.tensor([0] + [o for o in seqs[k].obj_ids if seqs[k].start_frame(o) <= t])
            assert len(ids) == K
            err = float((out[sid].cpu().double() - ref).abs().max())
            wrong = (pool.native_labels[sid].cpu().long() != ids[lab]) & ~excluded
            pixels[k] += int((lab > 0).sum())
            print('tick %d stream %d %r ragged %r%s: %d planes, max |soft - fp64| %.3e, excluded share %.5f, wrong labels %d, labels %r'
                  % (t, k, sizes[k], ragged, '' if eligible[sid] else ' FALLBACK', K, err, float(excluded.float().mean()), int(wrong.sum()), lab.unique().tolist()))
            assert err <= R.SOFT_TOL and float(excluded.float().mean()) <= R.EXCLUDED_CAP and int(wrong.sum()) == 0
    for sid in sids:
        pool.close(sid)
    assert fallbacks >= 1 and pixels[1] > 0 and pixels[2] > 0
