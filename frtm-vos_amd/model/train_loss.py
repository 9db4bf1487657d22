"""The loss tail of a refiner training step on HIP (csrc/train_step.hip: k_bce_logits): BCELoss(sigmoid(logits), target), its gradient
and the two counts of mask_iou from one pass over the logits, everything left on the device.

``bce_logits_stats(logits, target) -> (loss, inter, union)`` is differentiable in ``logits`` (from SegNetwork.forward_train or
forward_torch alike): the backward hands dz = (sigmoid(z) - t) / (N H W), scaled on the device by the loss's incoming gradient, to the
logits' grad_fn.  ``iou_from_counts`` finishes mask_iou's convention (an empty union counts as 1) from the integer counts.

Semantics: the loss is BCELoss(sigmoid(z), t) as a function of REAL numbers (softplus form, terms clamped at 100 like BCELoss's log).
The fp32 PyTorch composition differs for |z| > 16.6, where its sigmoid rounds to 1: DESIGN.md section 7."""
import torch

from .. import ops


class _BceLogitsStats(torch.autograd.Function):

    @staticmethod
    def forward(ctx, logits, target):
        loss, dz, inter, union = ops.bce_logits(logits, target, grad=ctx.needs_input_grad[0])
        ctx.dz = dz                                    # consumed (scaled in place) by the one backward pass
        ctx.mark_non_differentiable(inter, union)
        return loss, inter, union

    @staticmethod
    def backward(ctx, grad_loss, _gi, _gu):
        dz, ctx.dz = ctx.dz, None
        if dz is None:
            raise RuntimeError('bce_logits_stats: backward called twice (the gradient buffer is handed on, not kept)')
        return ops.scale_by_(dz, grad_loss.to(torch.float32)), None


def bce_logits_stats(logits, target):
    """logits (N,1,H,W) fp32 on the GPU, target of the same size (uint8 {0,1} or fp32 in [0,1]) -> (loss () fp32, inter (N) int32,
    union (N) int32), all device tensors.  CPU tensors raise RuntimeError (no CPU fallback), different sizes ValueError."""
    for name, t in (('logits', logits), ('target', target)):
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise RuntimeError('bce_logits_stats: %s is on %s; the loss kernel runs on the GPU only (no CPU fallback)' % (name, t.device))
    if tuple(logits.shape[-2:]) != tuple(target.shape[-2:]) or tuple(logits.shape) != tuple(target.shape):
        raise ValueError('bce_logits_stats: logits %s and target %s differ in size (resize the logits first: SegNetwork returns them '
                         'at the image size)' % (tuple(logits.shape), tuple(target.shape)))
    return _BceLogitsStats.apply(logits, target)


def iou_from_counts(inter, union):
    """mask_iou from its integer counts, per sample, on the device: inter / union, 1 where the union is empty.  (A handful of
    elements: N per frame.)"""
    u = union.to(torch.float32)
    return torch.where(union > 0, inter.to(torch.float32) / u.clamp(min=1), torch.ones_like(u))
