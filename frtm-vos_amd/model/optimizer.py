"""Gauss-Newton / conjugate-gradient solver (API of the reference's model/optimizer.py:5-160).

The reference obtains b = -J^T f0 and A p = J^T J p through ``torch.autograd.grad``
double-backward (optimizer.py:84,155-157) and runs the CG recurrences as dozens of tiny
TensorList ops with Python in between.  Here

 * the problem supplies explicit operators (``linearize`` -> b, ``apply_A`` -> q) that are a
   handful of fused HIP kernels each (see model/discriminator.py / csrc/target_model.hip);
 * all CG vectors (b, r, r_prev, p, q, delta) are slices of ONE flat device buffer and every
   scalar (rho, alpha, beta, <p,q>) stays on the device: ``run()`` enqueues kernels only and
   never synchronises;
 * the literal recurrences are kept, including their quirks:
   ``rho /= direction_forget_factor`` at the start of every run_CG once a direction exists
   (fp32, may overflow to inf => beta = 0), Polak-Ribiere beta clamped at 0, the skipped
   residual update on the last iteration, CG state carried across run() calls.
"""
import os

import torch

from .. import _hip as H
from ..lib.tensorlist import TensorList

HBAR_WORDS = 288        # FRTM_HBAR_WORDS of include/frtm_hip.h: int32 words of the resident solvers' XCD-hierarchical barrier state


class MinimizationProblem:
    """Protocol of a least-squares problem handled by GaussNewtonCG.

    HIP-backed problems implement:
      initialize()                  refresh views of the training data (reference discriminator.py:38-43)
      vector_layout() -> (n1, n2, diagM1, diagM2)   lengths / preconditioner of the two parameter parts
      linearize(x, b)               b <- -(J^T f(x) + lam^2 x)   (flat device vector)
      apply_A(p, q)                 q <- J^T J p + lam^2 p
      apply_step(x, step, delta)    x += step * delta (handles the internal layout)
      views(flat) -> TensorList     flat vector reshaped like the variables
    """

    def __call__(self, x: TensorList) -> TensorList:
        raise NotImplementedError

    def ip_input(self, a, b):
        return sum(a.view(-1) @ b.view(-1))

    def initialize(self):
        pass

    def M1(self, x):
        return x


def missed_iterations(launched, new_commits, new_aborts):
    """``num_cg_iter`` of the booked resident launches (oldest first) that neither committed nor were skipped by the guard, given how far the device's
    commit / abort counters rose over them.  Which ones is not recorded: the LAST are taken (the reference's update schedule has equal entries)."""
    missed = min(new_aborts, max(len(launched) - new_commits, 0))
    return launched[len(launched) - missed:] if missed > 0 else []


class ResidentLedger:
    """The host's books of one solver's resident launches over the device ``counters`` (GaussNewtonCG._gstats); ``mirror``: a pinned host word
    that follows the abort counter.  It only keeps books: which switches a time-out flips is its callers' business."""

    def __init__(self, counters, mirror):
        self.counters, self.mirror = counters, mirror
        self.launched = []           # num_cg_iter of the launches booked since the last settle (oldest first, the last 64)
        self.pending = False         # something has been booked since the last settle
        self.seen = (0, 0)           # (commits, aborts) at the last settle
        self.used = False            # a launch has been booked since the solver was rewound: THIS object's fit took the resident form

    def book(self, num_cg_iter, mirror=True):
        """A launch that has just been enqueued; ``mirror``: enqueue the copy of the abort counter that peek() looks at behind it."""
        self.pending = self.used = True
        self.launched.append(int(num_cg_iter))
        del self.launched[:-64]      # (bounded: callers that never settle -- benchmarks -- must not grow it)
        if mirror:
            self.mirror.copy_(self.counters[2:3], non_blocking=True)

    def book_replayed(self, schedule):
        """The resident launches of a run(schedule) that a replayed hipGraph has just enqueued (the graph holds no mirror copy)."""
        for n in (n for n in schedule if n > 0):
            self.book(n, mirror=False)

    def drop(self):
        """Forget (and hand back) what a hipGraph capture booked: it RECORDED those launches, the replays book the ones that run."""
        dropped, self.launched = self.launched, []
        return dropped

    def peek(self):
        """No wait: has the abort counter, as of the last mirror copy that landed, risen above the aborts already settled?"""
        return self.pending and int(self.mirror[0]) > self.seen[1]

    def settle(self):
        """The one synchronising read (16 bytes; none while nothing is pending): the missed iterations since the last call."""
        if not self.pending:
            return []
        launched, self.launched, self.pending = self.launched, [], False
        _, _, aborts, commits = self.counters.tolist()
        (commits0, aborts0), self.seen = self.seen, (commits, aborts)
        return missed_iterations(launched, commits - commits0, aborts - aborts0)

    def counts(self):
        return tuple(int(v) for v in self.counters[:2].tolist())

    def reset_counts(self):
        H.fill(self.counters[:2], 0)


class GaussNewtonCG:

    debug_abort = False              # tests (class or instance): the next persistent launches time out at their first barrier
    # Set (for the whole process) once a persistent launch has timed out: the GPU is shared with something that keeps this solver's
    # workgroups from becoming resident together, so new target models start in the multi-kernel form (Discriminator.init).
    abort_seen_in_process = False
    hierarchical_barrier = not os.environ.get('FRTM_FLAT_BARRIER')     # persistent launches: XCD-hierarchical grid barrier (False: one flat counter)
    persistent = False          # filter problem: run a whole GN iteration as one persistent launch (csrc/cg_persistent.hip) when the shape fits
    persistent_joint = True     # joint problem: resident form (csrc/joint_persistent.hip) where the problem offers it; switched off for the
                                # whole process once a launch has timed out (discriminator.leave_resident_forms)

    def __init__(self, problem: MinimizationProblem, variable: TensorList, cg_eps=0.0, fletcher_reeves=True,
                 standard_alpha=True, direction_forget_factor=0, step_alpha=1.0):
        # Problems with explicit operators (the target model's: DiscriminatorLoss) run on the fused HIP kernels.  Any other
        # MinimizationProblem -- user code written against the reference's protocol (__call__ / ip_input / M1, optimizer.py:5-15)
        # -- takes the generic form below: J p and J^T r through torch.autograd, exactly as the reference does it.  That form is
        # framework arithmetic on whatever device the problem's tensors live on; it is not the product's hot path.
        self._generic = not all(hasattr(problem, need) for need in ('vector_layout', 'linearize', 'apply_A', 'apply_step'))
        self._g = dict(p=None, rho=torch.ones(1), r_prev=None)
        self.fletcher_reeves = fletcher_reeves
        self.standard_alpha = standard_alpha
        self.direction_forget_factor = direction_forget_factor
        self.problem = problem
        self.x = variable
        self.cg_eps = cg_eps
        self.step_alpha = self._step_alpha0 = step_alpha
        self.residuals = torch.zeros(0)
        self.external_losses = []
        self.internal_losses = []
        self.gradient_mags = torch.zeros(0)
        self._n = None
        self._has_p = False
        self._buf = None
        self._pbuf = None                # exchange buffers of the filter problem's resident form (_filter_exchange)
        self._jbuf = None                # exchange buffers of the joint problem's resident form (_joint_exchange)
        self._guard = None               # (device count, minimum) while a guarded run() is in progress
        self._last_of_run = True         # the Gauss-Newton iteration being enqueued is the last of its run()
        self._gstats = None              # device int32[4]: guarded runs completed / skipped on the device, resident launches ABORTED / COMMITTED
        self.ledger = None               # ResidentLedger over _gstats (both exist from _stats() on): the host's books of the resident launches
        self._shadow = None              # snapshot of the solver state around a chain-form run with a device-side guard

    # ---- device state -------------------------------------------------------------------
    def _alloc(self):
        n1, n2, m1, m2 = self.problem.vector_layout()
        n = n1 + n2
        if self._buf is not None and self._n == n:
            return
        dev = self.x[0].device
        self._n, self._n1, self._n2 = n, n1, n2
        self._all = torch.zeros(6 * n + 8, device=dev)      # one allocation: a guarded chain-form run snapshots it with one copy
        self._buf = self._all[:6 * n].view(6, n)            # b, r, r_prev, p, q, delta
        self._state = self._all[6 * n:]
        self._state[:1].fill_(1.0)                          # rho = ones(1)  (optimizer.py:29); fill_, not a blocking indexed scalar store
        self._shadow = None
        self._partial = torch.zeros(4 * 64, device=dev)
        self._has_p = False
        # everything a launch may need exists BEFORE a caller opens a hipGraph capture around run(): the counters (+ their pinned mirror)
        # and, for a joint problem that can take the resident form, its exchange scratch (sized for the memory's capacity)
        self._stats()
        pr = self.problem
        if getattr(pr, 'joint', False) and hasattr(pr, 'persistent_joint_args'):
            self._joint_exchange(int(pr.mem.capacity), int(pr.Cin), int(pr.c), int(pr.h), int(pr.w))
        elif hasattr(pr, 'persistent_args'):
            self._filter_exchange()

    def _filter_exchange(self):
        """(slabs, qbuf, bar, hbar) of the filter problem's resident form, allocated once."""
        if self._pbuf is None:
            dev = self._buf.device
            self._pbuf = (torch.empty(256 * 864, device=dev), torch.zeros(864 + 256, device=dev), torch.zeros(4, dtype=torch.int32, device=dev),
                          torch.zeros(HBAR_WORDS, dtype=torch.int32, device=dev))
        return self._pbuf

    def _joint_exchange(self, N, Cin, c, h, w):
        """(scratch, bar, hbar) of the joint problem's resident form for N samples; grows, never shrinks.  A problem that does not fit the
        resident form (scratch size 0) allocates nothing."""
        need = int(H.lib().frtm_joint_persistent_scratch(N, Cin, c, h, w))
        if need > 0 and (self._jbuf is None or self._jbuf[0].numel() < need):
            dev = self._buf.device
            self._jbuf = (torch.empty(need, device=dev), torch.zeros(4, dtype=torch.int32, device=dev), torch.zeros(HBAR_WORDS, dtype=torch.int32, device=dev))
        return self._jbuf

    @property
    def b(self):
        if self._generic:
            return self._g.get('b')
        return None if self._buf is None else self.problem.views(self._buf[0])

    @property
    def p(self):
        if self._generic:
            return self._g['p']
        return self.problem.views(self._buf[3]) if self._has_p else None

    @property
    def r_prev(self):
        if self._generic:
            return self._g['r_prev']
        return self.problem.views(self._buf[2]) if self._has_p else None

    @property
    def rho(self):
        if self._generic:
            return self._g['rho']
        return torch.ones(1) if self._buf is None else self._state[0:1]

    def clear_temp(self):
        pass

    def rewind(self):
        """Back to the state of a newly constructed solver, keeping the device buffers (a recycled target model re-runs its
        first-frame fit through the same buffers, possibly as a replayed hipGraph: only device-side fills, no allocation)."""
        self._alloc()
        H.fill(self._all, 0.0)                              # _buf and _state are slices of this one allocation
        H.fill(self._state[:1], 1.0)
        self._has_p = self.ledger.used = False
        self.step_alpha = self._step_alpha0
        return self

    def reset_state(self):
        self._g.update(p=None, rho=torch.ones(1), r_prev=None)
        self._has_p = False
        if self._buf is not None:
            H.fill(self._state[:1], 1.0)

    # ---- solver ---------------------------------------------------------------------------
    def can_guard(self):
        """True if run() can take a device-side early-out (``guard``): every problem with HIP operators can -- persistent launches
        test the guard themselves, the multi-kernel chain is rolled back on the device when the guard says so."""
        return not self._generic

    def _stats(self):
        if self._gstats is None:
            self._gstats = torch.zeros(4, dtype=torch.int32, device=self.x[0].device)
            self.ledger = ResidentLedger(self._gstats, torch.zeros(1, dtype=torch.int32).pin_memory())
        return self._gstats

    def run(self, num_cg_iter, num_gn_iter=None, guard=None, guard_min=10):
        """``guard`` (device int32, one element): the whole run becomes a no-op ON THE DEVICE when its value is below ``guard_min`` --
        the reference's "fewer than 10 pixels" early-out (discriminator.py:214) without a device->host read.  Persistent launches
        return before their first barrier; a run in the multi-kernel form is executed on a snapshot basis: solver state and variables
        are copied aside first and copied back afterwards if the guard fails (4 tiny launches; the wasted solve is the rare case)."""
        self.problem.initialize()
        self._guard = None
        if guard is not None and self._generic:
            raise RuntimeError('GaussNewtonCG.run(guard=...): only for problems with HIP operators (can_guard())')
        if isinstance(num_cg_iter, int):
            if num_gn_iter is None:
                raise ValueError('Must specify number of GN iter if CG iter is constant')
            num_cg_iter = [num_cg_iter] * num_gn_iter
        if len(num_cg_iter) == 0:
            return None
        if self._generic:
            for n in num_cg_iter:
                self._generic_GN_iter(n)
            return self.external_losses, self.internal_losses, self.residuals
        self._alloc()
        chain_guard = False
        if guard is not None:
            self._guard = (guard, int(guard_min))
            # snapshot / roll-back covers every Gauss-Newton iteration that runs as a CHAIN of launches: all of them without a resident
            # plan, and the linearize-only entries (num_cg_iter == 0) even with one (those used to run unguarded).
            # Host-side state is NOT rolled back on a skipped solve: step_alpha *= 1.2 (capped at 1.0 -- the update solver starts at
            # 1.0, so nothing drifts) and _has_p = True with a zero direction on the device (p = z + 0 * beta: the same first step as
            # has_p = False).  The reference never enters run() on such a frame (discriminator.py:214).
            chain_guard = self._persistent_plan() is None or any(int(n) == 0 for n in num_cg_iter)
            if chain_guard:
                self._snapshot()
        try:
            for k, n in enumerate(num_cg_iter):
                self._last_of_run = k == len(num_cg_iter) - 1
                self.run_GN_iter(n)
        finally:
            self._guard = None
        if chain_guard:
            self._rollback_unless(guard, int(guard_min))
        return self.external_losses, self.internal_losses, self.residuals

    def _snapshot(self):
        n = self._all.numel() + sum(v.numel() for v in self.x)
        if self._shadow is None or self._shadow.numel() != n:
            self._shadow = torch.empty(n, device=self._all.device)
        o = self._all.numel()
        H.call('frtm_guarded_copy', H.ptr(self._shadow), H.ptr(self._all), o, None, 0, 0, None, 0)
        for v in self.x:
            H.call('frtm_guarded_copy', self._shadow.data_ptr() + 4 * o, H.ptr(v.data), v.numel(), None, 0, 0, None, 0)
            o += v.numel()

    def _rollback_unless(self, guard, guard_min):
        st = self._stats()
        o = self._all.numel()
        H.call('frtm_guarded_copy', H.ptr(self._all), H.ptr(self._shadow), o, guard.data_ptr(), guard_min, 1, H.ptr(st), 1)
        for v in self.x:
            H.call('frtm_guarded_copy', H.ptr(v.data), self._shadow.data_ptr() + 4 * o, v.numel(), guard.data_ptr(), guard_min, 1, None, 0)
            o += v.numel()

    def _persistent_joint_plan(self):
        pr = self.problem
        return pr.persistent_joint_args() if self.persistent_joint and hasattr(pr, 'persistent_joint_args') else None

    def _launch_flags(self):
        """Resets the CG state first if there is no forgetting factor, as every form of run_CG does; then the flags of its first direction
        update: (has_p, apply_dff, fletcher_reeves, standard_alpha, the factor rho is divided by)."""
        dff = float(self.direction_forget_factor)
        if dff == 0:
            self.reset_state()
        return int(self._has_p), int(self._has_p and dff != 0), int(self.fletcher_reeves), int(self.standard_alpha), dff or 1.0

    def _run_persistent_joint(self, num_cg_iter, a):
        """linearize + run_CG + apply_step of run_GN_iter for the JOINT problem: two small launches (transpose, Z = w1 X) + ONE resident
        launch.  Host-side bookkeeping as in run_CG."""
        pr = self.problem
        pr.prepare_linearization()
        scratch, bar, hbar = self._joint_exchange(a['N'], a['Cin'], a['c'], a['h'], a['w'])
        flags = self._launch_flags()
        n1, n2, m1, m2 = pr.vector_layout()
        H.call('frtm_joint_run_persistent', H.ptr(a['X']), H.ptr(a['Z']), H.ptr(a['B']), H.ptr(a['c_map']), H.ptr(a['sw']), a['N'], a['Cin'], a['c'],
               a['h'], a['w'], H.ptr(a['w1T']), H.ptr(a['w1']), H.ptr(a['w2']), H.ptr(self._buf), H.ptr(self._state), H.ptr(scratch), H.ptr(bar),
               H.ptr(hbar) if self.hierarchical_barrier else None, int(num_cg_iter), *flags, float(a['lam1']), float(a['lam2']), 1.0 / m1, 1.0 / m2,
               float(self.step_alpha), H.ptr(self._stats()), int(bool(self.debug_abort)))
        self._has_p = True
        self.ledger.book(num_cg_iter, mirror=False)     # (nobody peeks at a first-frame fit: Discriminator.init_aborted settles it)
        if hasattr(pr, '_invalidate_views'):
            pr._invalidate_views()

    def joint_aborts(self):
        """Aborted resident launches so far (stats[2]; 0 until THIS object's fit has launched in a resident form: solvers are pooled).  SYNCHRONISES;
        an aborted launch wrote nothing: that Gauss-Newton iteration is MISSING from the fit, the caller re-runs it in the chain form."""
        return int(self._gstats[2].item()) if self.ledger is not None and self.ledger.used else 0

    def _persistent_plan(self):
        pr = self.problem
        args = pr.persistent_args() if self.persistent and hasattr(pr, 'persistent_args') else None
        fits = args is not None and H.lib().frtm_cg_persistent_plan(args['N'], args['c'], args['h'], args['w'], None, None) > 0
        return args if fits else None

    def _run_persistent(self, num_cg_iter, a):
        """linearize + run_CG + apply_step of run_GN_iter in ONE launch; host-side bookkeeping as in run_CG."""
        slabs, qbuf, bar, hbar = self._filter_exchange()
        guard, guard_min = self._guard if self._guard is not None else (None, 0)
        flags = self._launch_flags()
        n1, n2, m1, m2 = self.problem.vector_layout()
        H.call('frtm_cg_run_persistent_guarded', H.ptr(a['X']), H.ptr(a['B']), H.ptr(a['c_map']), H.ptr(a['sw']), a['N'], a['c'], a['h'], a['w'],
               H.ptr(a['w2']), H.ptr(self._buf), H.ptr(self._state), H.ptr(slabs), H.ptr(qbuf), H.ptr(bar),
               int(num_cg_iter), *flags, float(a['lam2']), 1.0 / m1, float(self.step_alpha),
               None if guard is None else guard.data_ptr(), guard_min, H.ptr(self._stats()),
               int(guard is not None and self._last_of_run), int(bool(self.debug_abort)),
               H.ptr(hbar) if self.hierarchical_barrier else None)
        self._has_p = True
        self.ledger.book(num_cg_iter, mirror=not torch.cuda.is_current_stream_capturing())

    def replayed(self, schedule):
        """The host-side state an eager run leaves behind, after a hipGraph of one was replayed; ``schedule``: what ResidentLedger.drop handed back."""
        self._has_p = True
        self.ledger.book_replayed(schedule)

    def reset_persistent_counts(self):
        if self.ledger is not None:
            self.ledger.reset_counts()

    def persistent_counts(self):
        """(guarded runs completed, guarded runs that took the device-side early-out) so far.  SYNCHRONISES."""
        return (0, 0) if self.ledger is None else self.ledger.counts()

    def peek_persistent_abort(self):
        """No wait (ResidentLedger.peek; may lag by a launch).  True -> call poll_persistent_abort()."""
        return self.ledger is not None and self.ledger.peek()

    def poll_persistent_abort(self):
        """The ``num_cg_iter`` of the Gauss-Newton iterations that did NOT happen because their persistent launch gave up since the last poll (its
        workgroups could not all become resident within the spin time-out: the GPU is shared); empty: nothing to do.  An aborted launch leaves variable
        and solver state untouched (commit xor abort, cg_persistent.hip), so the CALLER re-runs exactly these (``run(missed)``; this solver is in the
        multi-kernel form from now on, and so is every solver created later in this process).  Launches skipped by the device-side guard are not missed.
        SYNCHRONISES (one 16-byte read); call it where the host waits anyway, or after peek_persistent_abort() said so."""
        if self.ledger is None:
            return []
        aborts, missed = self.ledger.seen[1], self.ledger.settle()
        if self.ledger.seen[1] > aborts:  # only the filter's form and the word for new target models (the joint form: leave_resident_forms)
            self.persistent = False
            GaussNewtonCG.abort_seen_in_process = True
        return missed

    def run_GN_iter(self, num_cg_iter):
        aj = self._persistent_joint_plan() if num_cg_iter > 0 else None
        a = self._persistent_plan() if num_cg_iter > 0 and aj is None else None
        if aj is not None:
            self._run_persistent_joint(num_cg_iter, aj)
        elif a is not None:
            self._run_persistent(num_cg_iter, a)
        else:
            self.problem.linearize(self.x, self._buf[0])
            if num_cg_iter > 0:
                self.run_CG(num_cg_iter)
                self.problem.apply_step(self.x, float(self.step_alpha), self._buf[5])
        self.step_alpha = min(self.step_alpha * 1.2, 1.0)

    def run_CG(self, num_iter, x=None, eps=0.0):
        if x is not None:
            raise NotImplementedError('warm-started CG (x != None) is never used by the reference call sites')
        pr = self.problem
        n1, n2, m1, m2 = pr.vector_layout()
        im1, im2 = 1.0 / m1, (1.0 / m2 if n2 else 1.0)
        b, r, r_prev, p, q, dx = [H.ptr(self._buf[i]) for i in range(6)]
        st, part = H.ptr(self._state), H.ptr(self._partial)
        has_p, apply_dff, fr, std_alpha, dff = self._launch_flags()
        H.call('frtm_cg_begin', b, r, r_prev, n1, n2, im1, im2, int(has_p and not fr), part)
        fused = n2 == 0 and n1 <= 1024 and hasattr(pr, 'apply_A_partials')
        if fused:
            # small single-tensor problem: one fused vector kernel per iteration (3 launches per CG iteration in total)
            H.call('frtm_cg_direction', r, p, n1, n2, im1, im2, has_p, apply_dff, fr, dff, st, part)
            self._has_p = True
            for ii in range(num_iter):
                slabs, nslab, stride, lam2 = pr.apply_A_partials(self._buf[3])
                H.call('frtm_cg_step_small', H.ptr(slabs), nslab, stride, float(lam2), dx, r, r_prev, p, q, n1, im1, int(ii == 0),
                       int(ii == num_iter - 1), std_alpha, fr, st)
            return pr.views(self._buf[5]), []
        for ii in range(num_iter):
            H.call('frtm_cg_direction', r, p, n1, n2, im1, im2, has_p if ii == 0 else 1, apply_dff if ii == 0 else 0, fr, dff, st, part)
            self._has_p = True
            if getattr(pr, 'joint', False) and hasattr(pr, 'has_pq') and pr.has_pq():
                # the problem's last kernel also leaves the partials of <p,q> (and <p,r>): no separate frtm_cg_pq launch
                pr.apply_A_pq(self._buf[3], self._buf[4], None if self.standard_alpha else self._buf[1], self._partial)
            else:
                pr.apply_A(self._buf[3], self._buf[4])
                H.call('frtm_cg_pq', p, q, None if self.standard_alpha else r, n1 + n2, part)
            H.call('frtm_cg_update', dx, r, r_prev, p, q, n1, n2, im1, im2, int(ii == 0), int(ii == num_iter - 1), std_alpha, st, part)
        return pr.views(self._buf[5]), []

    # ---- generic form: any MinimizationProblem, operators through autograd (reference optimizer.py:77-157) -------------------
    def _generic_GN_iter(self, num_cg_iter):
        x = self.x
        for v in x:
            v.requires_grad_(True)
        with torch.enable_grad():
            f0 = self.problem(x)                                                  # residual list
            g = TensorList([f.detach().clone().requires_grad_(True) for f in f0])
            jt_g = TensorList(torch.autograd.grad(list(f0), list(x), list(g), create_graph=True))     # J^T g, differentiable in g
        self._lin = (f0, g, jt_g)
        self._g['b'] = b = TensorList([-t.detach() for t in jt_g])
        delta = self._generic_CG(num_cg_iter, b) if num_cg_iter > 0 else []
        for v in x:
            v.detach_()
        for v, d in zip(x, delta):
            v.add_(d, alpha=float(self.step_alpha))
        self.step_alpha = min(self.step_alpha * 1.2, 1.0)
        self._lin = None

    def _generic_A(self, p):
        f0, g, jt_g = self._lin
        with torch.enable_grad():
            jp = torch.autograd.grad(list(jt_g), list(g), list(p), retain_graph=True)         # J p   (double backward, :156)
            return TensorList(torch.autograd.grad(list(f0), list(self.x), jp, retain_graph=True))   # J^T J p (incl. lam^2 p)

    def _generic_CG(self, num_iter, b):
        st, pr = self._g, self.problem
        dff = self.direction_forget_factor
        if dff == 0:
            self.reset_state()
        elif st['p'] is not None:
            st['rho'] = st['rho'] / dff                                           # may overflow to inf: beta = 0 (literal)
        r = TensorList([t.clone() for t in b])
        x = None
        for ii in range(num_iter):
            z = pr.M1(r)
            rho1, st['rho'] = st['rho'], pr.ip_input(r, z)
            if st['p'] is None:
                st['p'] = TensorList([t.clone() for t in z])
            else:
                beta = st['rho'] / rho1 if self.fletcher_reeves else (st['rho'] - pr.ip_input(st['r_prev'], z)) / rho1
                beta = beta.clamp(0)
                st['p'] = z + st['p'] * beta
            q = self._generic_A(st['p'])
            pq = pr.ip_input(st['p'], q)
            alpha = st['rho'] / pq if self.standard_alpha else pr.ip_input(st['p'], r) / pq
            if not self.fletcher_reeves:
                st['r_prev'] = TensorList([t.clone() for t in r])
            x = st['p'] * alpha if x is None else x + st['p'] * alpha
            if ii < num_iter - 1:
                r = r - q * alpha
        return x

    def A(self, x):
        """q = J^T J x + lam^2 x for a TensorList / flat vector in the problem's layout."""
        if self._generic:
            return self._generic_A(x)
        self._alloc()
        q = torch.empty(self._n, device=self._buf.device)
        flat = x if torch.is_tensor(x) else torch.cat([t.reshape(-1) for t in x])
        self.problem.apply_A(flat.contiguous(), q)
        return self.problem.views(q)

    def ip(self, a, b):
        return self.problem.ip_input(a, b)
