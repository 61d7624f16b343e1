"""The language-model loss of ``SPLMHeadModel.forward`` (models_sp.py:443-449: shift the logits, ``F.cross_entropy``) on the
library's row kernels: ``spq_lm_cross_entropy_fwd`` / ``spq_lm_cross_entropy_bwd`` (csrc/spq_lm_loss.hip).  The
logits are read where they lie -- no shifted copy, no ``log_softmax`` tensor -- and the backward writes ``softmax - onehot`` straight
into one full-size gradient.  ``SPLMHeadModel.forward`` uses it when ``use_hip_loss`` is set (``set_lm_loss``)."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib

REDUCTIONS = ('mean', 'sum', 'none')

# The kernels' plan (csrc/spq_lm_loss.hip): 256 threads per row, thread t owns the 4-element chunks t, t + 256, ... counted from
# the row's first element, four chunks loaded per thread and pass, thread 0 the V % 4 elements behind the last chunk.
CHUNK, ROW_THREADS, CHUNKS_PER_PASS = 4, 256, 4
# every V (up to three passes) at which that plan changes: thread 0 gets its first, second, third, fourth chunk (V = 4, 1028, 2052,
# 3076), the row needs a second pass (4100), a third (8196).  The vector width is 4 at every V; below 4 the row is all tail.
PLAN_CHANGES = tuple(CHUNK * (ROW_THREADS * k + 1) for k in (0, 1, 2, 3, CHUNKS_PER_PASS, 2 * CHUNKS_PER_PASS))


def plan_boundaries(V: int):
    """The element indices inside a row of ``V`` logits at which the plan passes from one owner to the next: a chunk to the next
    thread, a wavefront to the next, the last thread back to thread 0, one pass to the next, the last chunk to the scalar tail."""
    cuts = {CHUNK, CHUNK * 64, CHUNK * ROW_THREADS, CHUNK * ROW_THREADS * CHUNKS_PER_PASS, V - V % CHUNK}
    return tuple(sorted(c for c in cuts if 0 < c < V))


def served(logits: torch.Tensor, labels: torch.Tensor) -> bool:
    """Can ``lm_cross_entropy`` / ``token_nll`` take these tensors as they are (no copy, no cast)?  ``logits`` [B, T, V] or
    [rows, V] fp32, ``labels`` of the leading shape, int64; both on a GPU, contiguous and not empty."""
    return (logits.is_cuda and labels.is_cuda and logits.device == labels.device and logits.dtype == torch.float32
            and labels.dtype == torch.int64 and logits.dim() in (2, 3) and labels.shape == logits.shape[:-1]
            and logits.is_contiguous() and labels.is_contiguous() and logits.numel() > 0
            and logits.data_ptr() % 4 == 0 and labels.data_ptr() % 8 == 0)


def _require_served(what, logits, labels):
    _lib.require_gpu(logits, "logits")
    if not served(logits, labels):
        raise ValueError(f"{what}: needs contiguous, non-empty fp32 logits [B, T, V] (or [rows, V]) and int64 labels of the leading "
                         f"shape on the same device; got {tuple(logits.shape)} {logits.dtype} and {tuple(labels.shape)} "
                         f"{labels.dtype} on {labels.device} (served() tells beforehand)")
    _lib.check_device(logits.device)


def _shape(logits):
    return (1, logits.shape[0], logits.shape[1]) if logits.dim() == 2 else tuple(logits.shape)


def _forward(logits, labels, shift, ignore_index):
    """-> nll [B, T], lse [2, B, T] (value, rounding residual), loss [2] (sum, mean), count [1]; all on the device."""
    B, T, V = _shape(logits)
    dev = logits.device
    nll = torch.empty((B, T), dtype=torch.float32, device=dev)
    lse = torch.empty((2, B, T), dtype=torch.float32, device=dev)
    loss = torch.empty(2, dtype=torch.float32, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    with _lib.on_device(dev):
        rc = _lib.load().spq_lm_cross_entropy_fwd(logits.data_ptr(), labels.data_ptr(), B, T, V, int(shift), int(ignore_index),
                                                  nll.data_ptr(), lse.data_ptr(), loss.data_ptr(), count.data_ptr(),
                                                  _lib.stream_ptr(dev))
    _lib.check(rc, "spq_lm_cross_entropy_fwd")
    return nll, lse, loss, count


def _result(logits, nll, loss, shift, reduction):
    if reduction == 'mean':
        return loss[1]
    if reduction == 'sum':
        return loss[0]
    out = nll[:, :nll.shape[1] - int(shift)]
    return out[0] if logits.dim() == 2 else out


class _LMCrossEntropyFunction(torch.autograd.Function):
    """Saved: the logits and labels as they lie, the rows' log-sum-exp pair and the count -- nothing of size B T V."""

    @staticmethod
    def forward(ctx, logits, labels, shift, ignore_index, reduction):
        nll, lse, loss, count = _forward(logits, labels, shift, ignore_index)
        ctx.shift, ctx.ignore_index, ctx.reduction = shift, ignore_index, reduction
        ctx.save_for_backward(logits, labels, lse, count)
        return _result(logits, nll, loss, shift, reduction)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        logits, labels, lse, count = ctx.saved_tensors
        B, T, V = _shape(logits)
        g = g.contiguous().float()
        if g.numel() == 0:                                     # 'none' at T = 1 under the shift: no row counts, nothing is read
            g = g.new_zeros(1)
        per_row = ctx.reduction == 'none'
        dlogits = torch.empty_like(logits)
        with _lib.on_device(logits.device):
            rc = _lib.load().spq_lm_cross_entropy_bwd(logits.data_ptr(), labels.data_ptr(), lse.data_ptr(), B, T, V, int(ctx.shift),
                                                      int(ctx.ignore_index), None if per_row else g.data_ptr(),
                                                      g.data_ptr() if per_row else None,
                                                      count.data_ptr() if ctx.reduction == 'mean' else None, dlogits.data_ptr(),
                                                      _lib.stream_ptr(logits.device))
        _lib.check(rc, "spq_lm_cross_entropy_bwd")
        return dlogits, None, None, None, None


def lm_cross_entropy(logits: torch.Tensor, labels: torch.Tensor, shift: bool = True, ignore_index: int = -100,
                     reduction: str = 'mean') -> torch.Tensor:
    """``F.cross_entropy(logits[..., :-1, :].reshape(-1, V), labels[..., 1:].reshape(-1), ignore_index=..., reduction=...)`` with
    ``shift`` (the loss of models_sp.py:443-449), without it the same on ``logits`` and ``labels`` as given.  'none' returns the
    per-token values [B, T - shift] (0 where the label is ignored).  Records a gradient for ``logits`` (not twice differentiable);
    with gradients disabled, or logits that need none, only the forward runs.  Inputs that ``served`` rejects raise."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"lm_cross_entropy: reduction must be one of {REDUCTIONS}, got {reduction!r}")
    _require_served("lm_cross_entropy", logits, labels)
    shift = bool(shift)
    if torch.is_grad_enabled() and logits.requires_grad:
        return _LMCrossEntropyFunction.apply(logits, labels, shift, int(ignore_index), reduction)
    nll, _, loss, _ = _forward(logits.detach(), labels, shift, ignore_index)
    return _result(logits, nll, loss, shift, reduction)


def token_nll(logits: torch.Tensor, labels: torch.Tensor, shift: bool = True, ignore_index: int = -100) -> torch.Tensor:
    """The per-token negative log-likelihood [B, T - shift], no gradient: ``lm_cross_entropy(..., reduction='none')`` under
    ``no_grad``.  Its sum is the perplexity evaluators' ``reduction='sum'`` loss, its negative the log-probability the zero-shot
    scorer reads out of a ``log_softmax`` over the whole vocabulary."""
    with torch.no_grad():
        return lm_cross_entropy(logits, labels, shift=shift, ignore_index=ignore_index, reduction='none')
