"""The loss-side kernels of ContinuousPPOLearner (csrc/asg_ppo.hip) as tensor functions.

All of them work in the unroll kernels' flattened time-major row order -- [T, R, m] with
R = B * n, row = t * R + env * n + agent -- so the agent's logits, the critic's values, the
advantages and the gradients pass between them with no permute copy; the batch's own tensors
(bids [B, T, n, m], rewards [B, T, n], the mask [B, T]; batch- or time-major) are read through
their strides.  One launch each; no atomics, so two runs give the same bits."""
import ctypes

import torch

from .. import _lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _rows(x):
    """A [T, R, m] float32 buffer as the kernels read it (contiguous; a fresh tensor is 16-B aligned)."""
    x = x.float().contiguous()
    return x.clone() if x.data_ptr() % 16 != 0 else x


def _batch_args(bids, mask, n):
    """bids [B, T, n, m] and mask [B, T] with their {t, env, agent} element strides."""
    B, T, n_, m = bids.shape
    if n_ != n or tuple(mask.shape) != (B, T):
        raise ValueError(f"bids {tuple(bids.shape)} / mask {tuple(mask.shape)} do not fit n = {n}")
    if bids.dtype != torch.float32 or bids.stride(-1) != 1:
        bids = bids.float().contiguous()
    if mask.dtype != torch.float32:
        mask = mask.float()
    return (bids, _lib.i64arr([bids.stride(1), bids.stride(0), bids.stride(2)]), mask,
            _lib.i64arr([mask.stride(1), mask.stride(0), 0]), T, B, m)


def _log_prob_launch(logits, bids, mask, n, sigma, row_softmax):
    bids, bs, mask, ms, T, B, m = _batch_args(bids, mask, n)
    logits = _rows(logits)
    dev = logits.device
    logp = torch.empty((T, B * n, m), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().asg_bids_log_prob(_p(logits), _p(bids), bs, _p(mask), ms, T, B, n, m, float(sigma),
                                                int(bool(row_softmax)), _p(logp), _lib.stream_ptr(dev)))
    return logp


def bids_log_prob(logits, bids, mask, n, sigma, row_softmax):
    """Normal(bids, sigma).log_prob(pi) per element, [T, R, m]: pi = softmax(logits) per row
    (row_softmax) or the logits [T, R, m], and pi = 1 on the rows whose mask [B, T] is 0."""
    return _log_prob_launch(logits.detach(), bids, mask, n, sigma, row_softmax)


def _loss_launch(logits, bids, old_logp, adv, mask, inv_count, n, sigma, eps_clip, row_softmax, want_max):
    bids, bs, mask, ms, T, B, m = _batch_args(bids, mask, n)
    logits, old_logp, adv = _rows(logits), _rows(old_logp), _rows(adv)
    dev = logits.device
    N = T * B * n
    if inv_count.dtype != torch.float32 or inv_count.numel() != 1 or inv_count.device != dev:
        raise ValueError("inv_count is one float32 on the logits' device")
    groups = (N + _lib.ASG_PPO_ROWS_PER_GROUP - 1) // _lib.ASG_PPO_ROWS_PER_GROUP
    partial = torch.empty((groups,), dtype=torch.float32, device=dev)
    dlogits = torch.empty((T, B * n, m), dtype=torch.float32, device=dev)
    row_max = torch.empty((T, B * n), dtype=torch.float32, device=dev) if want_max else None
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().asg_ppo_bids_loss(
            _p(logits), _p(bids), bs, _p(old_logp), _p(adv), _p(mask), ms, T, B, n, m, float(sigma), float(eps_clip),
            _p(inv_count), int(bool(row_softmax)), _p(partial), _p(dlogits), _p(row_max), _lib.stream_ptr(dev)))
    return partial, dlogits, row_max


class _PPOBidsLoss(torch.autograd.Function):
    """asg_ppo_bids_loss under autograd: the forward launch computes the loss and its gradient
    with respect to the logits, the backward pass scales that gradient."""

    @staticmethod
    def forward(ctx, logits, bids, old_logp, adv, mask, inv_count, n, sigma, eps_clip, row_softmax, want_max):
        partial, dlogits, row_max = _loss_launch(logits, bids, old_logp, adv, mask, inv_count, n, sigma, eps_clip,
                                                 row_softmax, want_max)
        ctx.save_for_backward(dlogits)
        # the workgroups' sums, finished in one fixed-order reduction (float64: no rounding to speak of)
        loss = -(partial.sum(dtype=torch.float64).float() * inv_count.reshape(()))
        if row_max is None:
            return loss, None
        ctx.mark_non_differentiable(row_max)
        return loss, row_max

    @staticmethod
    def backward(ctx, grad_loss, _grad_max):
        dlogits, = ctx.saved_tensors
        return (grad_loss * dlogits,) + (None,) * 10


def ppo_bids_loss(logits, bids, old_logp, adv, mask, inv_count, n, sigma, eps_clip, row_softmax, want_max=False):
    """One epoch's clipped surrogate loss (reference learners/cont_ppo_learner.py:91-101) of the
    live logits [T, R, m], differentiable in them: -(min(ratio A, clamp(ratio, 1 - eps, 1 + eps) A)
    mask).sum() * inv_count, ratio = exp(log_prob(pi) - old_logp).  inv_count: a float32 device
    scalar, 1 / mask.sum() over the expanded mask.  Returns (loss, row maxima of pi [T, R] or None)."""
    return _PPOBidsLoss.apply(logits, bids, old_logp.detach(), adv.detach(), mask, inv_count, n, sigma, eps_clip,
                              row_softmax, want_max)


def _nstep_launch(values, rewards, mask, n, gamma, nsteps, add_value_last_step):
    B, T, n_ = rewards.shape
    values = _rows(values)
    m = values.shape[-1]
    if n_ != n or tuple(mask.shape) != (B, T) or tuple(values.shape) != (T + 1, B * n, m):
        raise ValueError(f"values {tuple(values.shape)} / rewards {tuple(rewards.shape)} / mask {tuple(mask.shape)} "
                         f"do not fit n = {n}")
    if rewards.dtype != torch.float32:
        rewards = rewards.float()
    if mask.dtype != torch.float32:
        mask = mask.float()
    dev = values.device
    out = torch.empty((T, B * n, m), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().asg_nstep_returns(
            _p(values), _p(rewards), _lib.i64arr([rewards.stride(1), rewards.stride(0), rewards.stride(2)]), _p(mask),
            _lib.i64arr([mask.stride(1), mask.stride(0), 0]), T, B, n, m, float(gamma), int(nsteps),
            int(bool(add_value_last_step)), _p(out), _lib.stream_ptr(dev)))
    return out


def nstep_returns(values, rewards, mask, n, gamma, nsteps, add_value_last_step):
    """The reference's nstep_returns (learners/cont_ppo_learner.py:174-192) on values [T + 1, R, m],
    rewards [B, T, n] and the mask [B, T]: [T, R, m]."""
    return _nstep_launch(values.detach(), rewards, mask, n, gamma, nsteps, add_value_last_step)
