"""BASELINE configs 4 and 5 against the CPU oracle (oracle/tracker_ref.py), not only against the product itself.

  (1) config 5 (1080x1920, ResNet-101, 8 objects, memory 32), one tracker step teacher-forced like the 720p test of test_north_star_gpu.py:
      68x120 score maps, the strip kernels of csrc/wide_maps.hip, the chain-form re-solve with its device-side guard, 9-plane merges.
  (2) config 4 (720p, 3 objects, the last one entering on frame 5), teacher-forced ACROSS the entry frame: the late-entry rules of the reference
      (tracker.py:136-141, 165-191, 193-227) -- initialize() zeroes the old planes, the old objects' refiner outputs are multiplied by
      (1 - start mask) of the new one, the new object is neither scored nor updated on its start frame, the old ones insert the merged masks.
  (3) the same sequence free-running through the three tracker paths (Tracker.run_sequence, the literal per-frame loop) and
      TrackerRef.run_sequence.
"""
import time

import pytest
import torch

from oracle import cpu_ref as O
from oracle import make_golden_jf as JF
from oracle.tracker_ref import TrackerRef
from test_north_star_gpu import DEV, _hip_tracker, _teacher_forced, cpu_threads

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(1800)]

LATE = dict(size=(720, 1280), n_frames=8, n_obj=3, seed=6, late_object_at=5)


def _gates(worst):
    """The 720p teacher-forced test's gates (test_north_star_gpu.py: test_teacher_forced_step_at_720p_wide_maps)."""
    assert worst['raw'] <= 1e-3 and worst['merged'] <= 1e-3, worst
    assert worst['filt'] == 0.0 and worst['sw'] <= 1e-6, worst
    assert worst['arb_pooled'] <= 1.5 and worst['arb'] <= 2.0, worst
    assert sum(1 for v in worst['arb_each'] if v > 1.5) <= 1, worst['arb_each']


def test_config5_1080p_eight_objects_teacher_forced():
    """Config 5 at full size: frame 0 initialises 8 objects (joint fits on 68x120 maps), 2 tracked frames with train_skipping = 2, so every
    object re-solves once (frame 2).  Gates of the 720p test; and the path is the wide one: the strip forms on every object's problems,
    the re-solve in the multi-kernel chain (the persistent CG launch is not eligible at w = 120) under its device-side guard, 9 planes merged."""
    from frtm_vos_amd import _hip as H
    t0 = time.time()
    disc = dict(JF.DISC, train_skipping=2, memory_size=32)
    solved_by = {}

    def check(t, trk, cpu, solved):
        assert trk.current_masks.shape == cpu.current_masks.shape == (9, 1080, 1920)
        assert len(trk._raw_log[-1][1]) == 9
        for oid in solved:
            solved_by[oid] = t
        for oid, tg in trk.targets.items():
            d = tg.discriminator
            opt, prob = d.update_optimizer, d.update_optimizer.problem
            assert prob.wide_parts > 0 and d._init_opt.problem.wide_parts > 0, (oid, prob.wide_parts)
            assert (prob.h, prob.w) == (68, 120) and d.memory.capacity == 32
            if oid in solved:
                a = prob.persistent_args()
                assert H.lib().frtm_cg_persistent_plan(a['N'], a['c'], a['h'], a['w'], None, None) <= 0, oid
                assert not opt.ledger.pending and not opt.ledger.launched, oid          # no resident launch: the chain ran
                assert opt._shadow is not None, oid                                     # ... under the device-side guard (snapshot taken)
                assert d.num_solves == 1 and d.num_early_outs == 0, (oid, d.num_solves, d.num_early_outs)

    worst = _teacher_forced((1080, 1920), 3, 8, 302, disc, check=check, threads=cpu_threads())
    print('config 5 teacher-forced: re-solve frame per object %s, %.0f s' % (solved_by, time.time() - t0))
    assert solved_by == {oid: 2 for oid in range(1, 9)}, solved_by
    _gates(worst)


def test_config4_late_object_teacher_forced_across_entry():
    """720x1280, ResNet-101, 3 objects, object 3 enters on frame 5; frames 0-7, memory 16, train_skipping = 2.  The old objects' state is
    forced before every frame, the new one's from frame 6 on.  On frame 5 (inside the helper): initialize() leaves the oracle's planes, the
    same object-to-plane order, the new object's fit within 0.3 rms, its plane before the merge = its label mask exactly, the old planes zero
    under that mask, its target model untouched by the frame; the pre-merge and merged planes within 1e-3.  Every frame: the gates of the
    720p test.  Old objects re-solve on frames 2, 4, 6, the new one on frame 7."""
    t0 = time.time()
    disc = dict(JF.DISC, train_skipping=2, memory_size=16)
    solves = {}

    def check(t, trk, cpu, solved):
        solves[t] = sorted(solved)
        if t == LATE['late_object_at']:
            assert trk.current_masks.shape[0] == cpu.current_masks.shape[0] == 4
            assert {oid: tg.index for oid, tg in trk.targets.items()} == {oid: ct['index'] for oid, ct in cpu.targets.items()} == {1: 1, 2: 2, 3: 3}

    worst = _teacher_forced(LATE['size'], LATE['n_frames'], LATE['n_obj'], LATE['seed'], disc, late_object_at=LATE['late_object_at'], check=check,
                            threads=cpu_threads())
    print('config 4 teacher-forced across the entry frame: entry frame max |mask diff| before merge %.2e, merged %.2e; re-solves %s; %.0f s'
          % (worst['entry_raw'], worst['entry_merged'], solves, time.time() - t0))
    assert worst['entry_raw'] <= 1e-3 and worst['entry_merged'] <= 1e-3, worst
    assert solves == {1: [], 2: [1, 2], 3: [], 4: [1, 2], 5: [], 6: [1, 2], 7: [3]}, solves
    _gates(worst)


def test_config4_late_object_free_running_three_paths():
    """The same sequence free-running: Tracker.run_sequence (windows, batched trunk, graphs), the literal per-frame loop (initialize() then
    track() on the entry frame, reference tracker.py:136-141) and TrackerRef.run_sequence.  Each HIP path agrees with the oracle on > 99.5 %
    of the labels of the tracked frames; object 3 is absent from frames 0-4 and holds more than 10 pixels on the last frame in all three."""
    from frtm_vos_amd import ops
    from frtm_vos_amd.lib.synthetic import SyntheticSequence
    torch.set_grad_enabled(False)
    torch.set_num_threads(cpu_threads())
    t0 = time.time()
    size, seed, late = LATE['size'], LATE['seed'], LATE['late_object_at']
    seq = SyntheticSequence('late', LATE['n_frames'], size, LATE['n_obj'], seed=seed, late_object_at=late)
    refiner = JF.refiner_for('resnet101')
    disc = dict(JF.DISC, train_skipping=2, memory_size=16)
    over = {k: v for k, v in disc.items() if JF.DISC.get(k) != v}
    start = lambda oid: JF.start_weights(seed, oid)
    cpu = TrackerRef('resnet101', O.resnet_random_params('resnet101', seed=0), refiner, start, **disc)
    ref = torch.stack([l.reshape(size) for l in cpu.run_sequence(seq)])
    t_cpu = time.time() - t0

    trk = _hip_tracker('resnet101', refiner, **over)
    trk.start_weights = start
    seq.preload(DEV)
    fast, _ = trk.run_sequence(seq)
    fast = torch.stack([l.reshape(size) for l in fast]).cpu()

    trk = _hip_tracker('resnet101', refiner, **over)
    trk.start_weights = start
    ids = torch.tensor([0] + list(seq.obj_ids), dtype=torch.uint8, device=DEV)
    trk.current_frame, trk.targets = 0, dict()
    slow = []
    for image, labels, new in seq:
        had = len(trk.targets) > 0
        if new:
            trk.initialize(image, labels.to(DEV), new)
        if had:
            labels = ids[ops.merge_masks_(trk.track(image).clone()).argmax(dim=0, keepdim=True)]
        slow.append(labels.reshape(size).cpu())
        trk.current_frame += 1
    slow = torch.stack(slow)
    seq.release()

    agree = {name: float((lab[1:] == ref[1:]).float().mean()) for name, lab in (('run_sequence', fast), ('literal loop', slow))}
    print('config 4 free-running, label agreement with TrackerRef over frames 1-%d: %s; object 3 pixels on the last frame: oracle %d, run_sequence %d, '
          'literal loop %d  (oracle %.0f s, total %.0f s)' % (len(ref) - 1, {k: round(v, 5) for k, v in agree.items()}, int((ref[-1] == 3).sum()),
                                                            int((fast[-1] == 3).sum()), int((slow[-1] == 3).sum()), t_cpu, time.time() - t0))
    for name, lab in (('oracle', ref), ('run_sequence', fast), ('literal loop', slow)):
        assert int((lab[:late] == 3).sum()) == 0, name
        assert int((lab[-1] == 3).sum()) > 10, name
    assert min(agree.values()) > 0.995, agree
