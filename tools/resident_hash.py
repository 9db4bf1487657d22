"""sha256 of what the two resident solver launches leave behind (k_cg_run_persistent, k_joint_run_persistent), for an A/B of two builds of
the library that must not differ in a bit:  python tools/resident_hash.py [path/to/libfrtm_hip.so] [--time]   (one process per library; diff the outputs).

Filter problem at the shapes of test_persistent_cg_run_equals_the_multi_kernel_form / _single_step_is_tight, joint problem at the shapes of
test_resident_joint_fit_equals_the_chain_form; each with the hierarchical and the flat barrier, Polak-Ribiere and Fletcher-Reeves, a first run
(no carried direction) and a second (carried direction, forgetting factor applied); the filter problem also through a guarded launch that
skips and one that runs.  The kernels are deterministic, so one unequal hash is a changed order of operations, not noise.

--time: instead of the hashes, device-event times of the resident filter re-solve run((10,)) on a full 80-sample 480p memory (what bench.py's
roofline_cg leg reports) and of one Gauss-Newton iteration (10 CG steps) of the joint fit (5 samples, 1024 -> 96 channels, 30x54)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from frtm_vos_amd import _hip as H  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
if args:
    H.LIB_PATH = os.path.abspath(args[0])          # before the first call loads it
from test_round2_gpu import _filter_problem  # noqa: E402
from test_round4_gpu import _joint_case  # noqa: E402

FILTER_SHAPES = [(80, 96, 30, 54, 480, 854), (32, 96, 30, 54, 480, 854), (7, 8, 6, 9, 48, 70), (5, 96, 30, 54, 480, 854), (24, 40, 17, 31, 272, 496),
                 (3, 16, 23, 64, 184, 512), (13, 96, 30, 54, 480, 854)]
JOINT_SHAPES = [(1024, 96, 30, 54, 480, 854), (256, 96, 30, 54, 480, 854), (200, 40, 17, 31, 272, 496), (64, 16, 12, 64, 96, 512)]


def sha(*tensors):
    torch.cuda.synchronize()
    return ' '.join(hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:16] for t in tensors)


def hashes():
    for shape in FILTER_SHAPES:
        for hier in (True, False):
            for fr in (False, True):
                mem, opt, wv, g = _filter_problem(*shape, 11, True, dff=0.9 ** 75)
                opt.hierarchical_barrier, opt.fletcher_reeves = hier, fr
                for run, sched in enumerate(((10,), (5,))):
                    opt.run(sched)
                    print('filter', shape, 'hier' if hier else 'flat', 'FR' if fr else 'PR', 'run', run, sha(wv, opt._buf, opt._state, opt._stats()))
                assert opt.ledger.pending and not opt.poll_persistent_abort()
                for count in (3, 50):                     # below / above guard_min = 10: the launch returns at once / runs
                    opt.run((3,), guard=torch.tensor([count], dtype=torch.int32, device=wv.device))
                    print('filter', shape, 'hier' if hier else 'flat', 'FR' if fr else 'PR', 'guard', count, sha(wv, opt._buf, opt._state, opt._stats()))
    for shape in JOINT_SHAPES:
        for hier in (True, False):
            for fr in (False, True):
                mem, prob, opt, w1, w2 = _joint_case(*shape, 3, True)
                opt.direction_forget_factor = 0.9 ** 75
                opt.hierarchical_barrier, opt.fletcher_reeves = hier, fr
                prob.initialize()
                assert opt._persistent_joint_plan() is not None
                for run, sched in enumerate(((5,), (3, 3))):
                    opt.run(sched)
                    print('joint', shape, 'hier' if hier else 'flat', 'FR' if fr else 'PR', 'run', run, sha(w1, w2, opt._buf, opt._state, opt._stats()))
                assert opt.joint_aborts() == 0


def timed(fn, budget_ms=300.0):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    reps = max(10, int(budget_ms / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps, reps


def times():
    mem, opt, wv, g = _filter_problem(80, 96, 30, 54, 480, 854, 11, True)
    us, reps = timed(lambda: opt.run((10,)))
    assert not opt.poll_persistent_abort()
    print('filter run((10,)) N=80 96ch 30x54: %.2f us per run (%d runs)' % (us, reps))
    mem, prob, opt, w1, w2 = _joint_case(1024, 96, 30, 54, 480, 854, 3, True)
    prob.initialize()
    assert opt._persistent_joint_plan() is not None
    us, reps = timed(lambda: opt.run((10,)))
    assert opt.joint_aborts() == 0
    print('joint run((10,)) N=5 1024->96ch 30x54: %.2f us per Gauss-Newton iteration (%d runs)' % (us, reps))


with torch.no_grad():
    H.lib()
    print('library:', [ln.split()[-1] for ln in open('/proc/self/maps') if 'libfrtm_hip' in ln][0], file=sys.stderr)      # (stderr: the outputs stay comparable)
    times() if '--time' in sys.argv else hashes()
