"""torch.optim.Adam with its step on HIP (csrc/train_step.hip: k_adam): one launch per parameter group instead of the foreach path's
dozen launches over lists of 116 tensors.

Everything but ``step()`` is torch's own: the state tensors and their lazy creation (``Adam._init_group``), ``state_dict()`` /
``load_state_dict()`` (step, exp_avg, exp_avg_sq, max_exp_avg_sq), ``param_groups`` -- so lr schedulers work unchanged and a checkpoint
written with either optimiser loads into the other.  The update is Adam's documented one with weight_decay folded into the gradient
and optional AMSGrad, per element in fp32.

The kernel walks a device table of (param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, count) per tensor; lr, the bias corrections,
betas, eps and weight_decay are launch arguments.  The table is rebuilt only when a pointer in it changes (first step, a reallocated
gradient, a different set of parameters with gradients, a loaded state), never by a scheduler."""
import torch

from .. import _hip as H
from .. import ops


class FusedAdam(torch.optim.Adam):

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, **kwargs):
        self._refuse(dict(kwargs, lr=lr))
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kwargs)
        self._tables = {}              # (group index, rank of the step count within the group) -> (key, tensors, chunks, n_tensors, n_chunks)

    @staticmethod
    def _refuse(group):
        """What torch.optim.Adam offers and the kernel does not do (constructor arguments, or a parameter group of a loaded state)."""
        for flag in ('maximize', 'capturable', 'differentiable', 'fused', 'foreach', 'decoupled_weight_decay'):
            if group.get(flag):
                raise ValueError('FusedAdam does not implement %s=True (torch.optim.Adam does)' % flag)
        if isinstance(group['lr'], torch.Tensor):
            raise ValueError('FusedAdam takes the learning rate as a Python float (it is a launch argument)')

    @staticmethod
    def _check(p, g):
        if not p.is_cuda:
            raise RuntimeError('FusedAdam: parameter on %s; the optimiser step runs on the GPU only (no CPU fallback)' % (p.device,))
        if g.is_sparse:
            raise RuntimeError('FusedAdam does not support sparse gradients')
        if p.dtype != torch.float32 or g.dtype != torch.float32:
            raise TypeError('FusedAdam: fp32 parameters and gradients only, got %s / %s' % (p.dtype, g.dtype))
        if not p.is_contiguous() or not g.is_contiguous():
            raise ValueError('FusedAdam: parameters and gradients must be contiguous (shape %s)' % (tuple(p.shape),))
        if g.device != p.device or g.shape != p.shape:
            raise ValueError('FusedAdam: gradient %s on %s for a parameter %s on %s' % (tuple(g.shape), g.device, tuple(p.shape), p.device))
        if p.device.index != torch.cuda.current_device():
            raise RuntimeError('FusedAdam: parameter on %s but the current device is cuda:%d' % (p.device, torch.cuda.current_device()))

    def _table(self, slot, rows):
        """Device tables for ``rows`` = [(p, g, m, v, vmax or None)], cached under ``slot`` while no pointer changes."""
        key = tuple((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if x is None else x.data_ptr(), p.numel())
                    for p, g, m, v, x in rows)
        hit = self._tables.get(slot)
        if hit is not None and hit[0] == key:
            return hit
        E = ops.adam_chunk_elems()
        words, chunks = [], []
        for k in key:
            if k[5] == 0:
                continue
            aligned = all(a % 16 == 0 for a in k[:5])
            words += list(k) + [int(aligned), 0]
            t = len(words) // 8 - 1
            chunks += [c for j in range((k[5] + E - 1) // E) for c in (t, j)]
        dev = rows[0][0].device
        n_t, n_c = len(words) // 8, len(chunks) // 2
        hit = (key, H.upload(torch.tensor(words, dtype=torch.int64), dev) if n_t else None,
               H.upload(torch.tensor(chunks, dtype=torch.int32), dev) if n_c else None, n_t, n_c)
        self._tables[slot] = hit
        return hit

    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        with torch.no_grad():
            for gi, group in enumerate(self.param_groups):
                self._refuse(group)
                for p in group['params']:
                    if p.grad is not None:
                        self._check(p, p.grad)
                params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps = [], [], [], [], [], []
                self._init_group(group, params, grads, exp_avgs, exp_avg_sqs, max_sqs, steps)       # torch's own lazy state
                if not params:
                    continue
                ams = bool(group['amsgrad'])
                beta1, beta2 = group['betas']
                by_step = {}                                          # parameters that skipped steps (grad None) have their own count
                for i, s in enumerate(steps):
                    s += 1
                    by_step.setdefault(int(s), []).append(i)
                for k, (t, idx) in enumerate(sorted(by_step.items())):
                    rows = [(params[i], grads[i], exp_avgs[i], exp_avg_sqs[i], max_sqs[i] if ams else None) for i in idx]
                    for r in rows:
                        for x in r[2:]:
                            if x is not None and (not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous()):
                                raise ValueError('FusedAdam: optimiser state must be contiguous fp32 on the GPU')
                    _, tensors, chunks, n_t, n_c = self._table((gi, k), rows)
                    if n_t == 0:
                        continue
                    ops.adam_step(tensors, n_t, chunks, n_c, group['lr'], 1.0 - beta1 ** t, 1.0 - beta2 ** t, beta1, beta2, group['eps'],
                                  group['weight_decay'], ams)
        return loss
