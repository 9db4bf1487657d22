"""The host's books of the resident solver launches (model/optimizer.py: ResidentLedger, missed_iterations), without a GPU: a CPU int32[4]
tensor stands in for the device counters [guarded runs completed, skipped, launches ABORTED, launches COMMITTED], a plain CPU word for
the pinned mirror of the abort counter.

The expected values of ROWS were recorded from poll_persistent_abort() as it was before the ledger existed (its privates
_persistent_launched / _launched / _committed_seen / _aborts_handled set by hand on such a tensor); the rows were then ported unchanged."""
import pytest
import torch

from frtm_vos_amd.lib.tensorlist import TensorList
from frtm_vos_amd.model.optimizer import GaussNewtonCG, MinimizationProblem, ResidentLedger, missed_iterations


class Counters:
    """The stand-in for the device counters; counts the synchronising reads (on the device, tolist() is the one that waits)."""

    def __init__(self, commits=0, aborts=0):
        self.t = torch.tensor([0, 0, aborts, commits], dtype=torch.int32)
        self.reads = 0

    def tolist(self):
        self.reads += 1
        return self.t.tolist()

    def __getitem__(self, k):
        return self.t[k]


# booked | counters rise by (commits, aborts) | (commits, aborts) seen before | missed | filter form switched off
ROWS = [
    ([10, 10, 10], (3, 0), (0, 0), [], False),
    ([10, 10, 10], (2, 1), (0, 0), [10], True),
    ([5, 10, 10], (1, 2), (0, 0), [10, 10], True),
    ([4, 4], (0, 2), (0, 0), [4, 4], True),
    ([10, 10], (1, 0), (0, 0), [], False),           # one skipped by the guard: neither commits nor aborts
    ([10, 10], (1, 1), (0, 0), [10], True),          # one skipped, one aborted
    ([10], (1, 1), (0, 0), [], True),                # abort of a launch that was not booked
    ([], (0, 1), (0, 0), [], True),                  # pending, nothing booked: after a capture dropped its bookings
    ([5, 10], (0, 1), (7, 3), [10], True),
    ([5, 10], (1, 3), (7, 3), [10], True),
]


def _ledger(booked, rise, seen):
    c = Counters(seen[0], seen[1])
    led = ResidentLedger(c, torch.zeros(1, dtype=torch.int32))
    led.seen = tuple(seen)
    for n in booked:
        led.book(n, mirror=False)
    if not booked:
        led.book(10, mirror=False)      # what a hipGraph capture leaves: its bookings dropped, the ledger still pending
        assert led.drop() == [10]
    assert led.pending and led.launched == booked and c.reads == 0
    c.t[3] += rise[0]
    c.t[2] += rise[1]
    return led, c


@pytest.mark.parametrize('booked,rise,seen,missed,off', ROWS)
def test_settle_returns_the_missed_iterations_once_and_moves_seen_up_to_the_counters(booked, rise, seen, missed, off):
    led, c = _ledger(booked, rise, seen)
    assert missed_iterations(list(booked), *rise) == missed                    # the arithmetic alone: no device, no solver
    assert led.settle() == missed and c.reads == 1
    assert led.seen == (seen[0] + rise[0], seen[1] + rise[1]) and (led.seen[1] > seen[1]) is off
    assert not led.pending and led.launched == []
    assert led.settle() == [] and c.reads == 1, 'a second settle without a new booking read the counters'
    assert led.seen == (seen[0] + rise[0], seen[1] + rise[1])


@pytest.mark.parametrize('booked,rise,seen,missed,off', ROWS)
def test_poll_switches_off_the_filter_form_and_nothing_else(booked, rise, seen, missed, off):
    """poll_persistent_abort() on a solver that owns such a ledger: the same missed iterations; a time-out turns off ``persistent`` and sets
    ``abort_seen_in_process`` -- the joint form (``persistent_joint``) stays as it is."""
    saved = GaussNewtonCG.abort_seen_in_process, GaussNewtonCG.persistent_joint
    try:
        GaussNewtonCG.abort_seen_in_process = False
        opt = GaussNewtonCG(MinimizationProblem(), TensorList([torch.zeros(1)]))
        opt.persistent = True
        opt.ledger, c = _ledger(booked, rise, seen)
        opt._gstats = c
        assert opt.poll_persistent_abort() == missed and c.reads == 1
        assert opt.persistent is (not off) and GaussNewtonCG.abort_seen_in_process is off
        assert GaussNewtonCG.persistent_joint is saved[1] and 'persistent_joint' not in vars(opt)
        assert opt.poll_persistent_abort() == [] and c.reads == 1
    finally:
        GaussNewtonCG.abort_seen_in_process, GaussNewtonCG.persistent_joint = saved


def test_seventy_bookings_keep_the_last_64():
    led = ResidentLedger(Counters(), torch.zeros(1, dtype=torch.int32))
    for n in range(70):
        led.book(n + 1, mirror=False)
    assert led.launched == list(range(7, 71)) and led.pending


def test_a_replayed_schedule_is_booked_like_an_eager_launch_without_the_mirror():
    def state(led):
        return led.launched, led.pending, led.seen, int(led.mirror[0])
    a, b = (ResidentLedger(Counters(aborts=2), torch.zeros(1, dtype=torch.int32)) for _ in range(2))
    a.book_replayed((10,))
    b.book(10, mirror=False)
    assert state(a) == state(b) == ([10], True, (0, 0), 0) and a.used and b.used       # (the mirror word untouched: no copy was enqueued)
    a.book_replayed((0, 5, 0, 10))                                  # linearize-only entries launch nothing resident: not booked
    assert a.launched == [10, 5, 10]


def test_peek_follows_the_mirror_word_not_the_counters():
    c = Counters(commits=4, aborts=3)
    led = ResidentLedger(c, torch.zeros(1, dtype=torch.int32))
    led.seen = (4, 3)
    c.t[2] += 1
    assert not led.peek()                       # nothing pending
    led.book(10, mirror=False)
    assert not led.peek()                       # the mirror word has not risen above the aborts already settled
    led.mirror[0] = 3
    assert not led.peek()
    led.book(10)                                # with the mirror copy: the word follows the abort counter
    assert int(led.mirror[0]) == 4 and led.peek() and c.reads == 0
    assert led.settle() == [10] and not led.peek()
