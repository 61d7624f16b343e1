"""The causal attention core between c_attn and c_proj (models_sp.py:61-75) as one HIP launch: ``spq_causal_attention_fwd``
(csrc/spq_attention.hip), and its backward ``spq_causal_attention_bwd`` (csrc/spq_attention_bwd.hip, DESIGN.md
3.14) behind ``causal_attention_autograd``.  ``SPAttention.core`` uses the forward when ``use_hip_core`` is set and, under a
gradient, the pair when ``use_hip_backward`` is set as well."""
import torch
from torch.autograd.function import once_differentiable

from . import _lib

HEAD_DIMS = (16, 32, 64, 80, 128)         # what spq_causal_attention_fwd serves; 64 is every GPT-2 size
BWD_HEAD_DIMS = (16, 32, 64)              # what spq_causal_attention_bwd serves


def served(qkv: torch.Tensor, n_head: int) -> bool:
    """Can ``causal_attention`` take this tensor as it is (no copy, no cast)?"""
    return (qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 3 and qkv.is_contiguous() and qkv.numel() > 0
            and qkv.shape[2] % (3 * n_head) == 0 and qkv.shape[2] // (3 * n_head) in HEAD_DIMS and qkv.data_ptr() % 16 == 0)


def served_backward(qkv: torch.Tensor, n_head: int) -> bool:
    """Can ``causal_attention_autograd`` take this tensor as it is, forward and backward?"""
    return served(qkv, n_head) and qkv.shape[2] // (3 * n_head) in BWD_HEAD_DIMS


def causal_attention(qkv: torch.Tensor, n_head: int, return_lse: bool = False):
    """``qkv`` [B, T, 3C] (c_attn's output: q | k | v along the last dimension, head h at columns h*d of each third) ->
    ``out`` [B, T, C] with the heads merged; with ``return_lse`` also the rows' log-sum-exp [B, n_head, T] (natural log of the
    sum over j <= t of exp(q.k_j / sqrt(d))).  No gradient is recorded.  fp32, contiguous, on a gfx950 device; a shape the
    kernel does not serve raises (there is no fallback here -- ``SPAttention.core`` chooses the path)."""
    _lib.require_gpu(qkv, "qkv")
    if qkv.dim() != 3 or qkv.shape[2] % (3 * n_head) != 0:
        raise ValueError(f"causal_attention: qkv must be [B, T, 3 * n_head * head_dim], got {tuple(qkv.shape)} for n_head={n_head}")
    if not qkv.is_contiguous():
        raise ValueError("causal_attention: qkv must be contiguous (c_attn's output as it lies in memory)")
    _lib.check_device(qkv.device)
    B, T, C3 = qkv.shape
    C = C3 // 3
    qkv = qkv.detach()
    out = torch.empty((B, T, C), dtype=torch.float32, device=qkv.device)
    lse = torch.empty((B, n_head, T), dtype=torch.float32, device=qkv.device) if return_lse else None
    with _lib.on_device(qkv.device):
        rc = _lib.load().spq_causal_attention_fwd(qkv.data_ptr(), B, T, n_head, C // n_head, out.data_ptr(), _lib.ptr(lse),
                                                  _lib.stream_ptr(qkv.device))
    _lib.check(rc, "spq_causal_attention_fwd")
    return (out, lse) if return_lse else out


class _CausalAttentionFunction(torch.autograd.Function):
    """``spq_causal_attention_fwd`` with ``spq_causal_attention_bwd`` as its backward.  Saved: qkv as it lies (no copies of q, k
    or v), the output and the rows' log-sum-exp; the probabilities are recomputed.  fp32 only."""

    @staticmethod
    def forward(ctx, qkv, n_head):
        out, lse = causal_attention(qkv, n_head, return_lse=True)
        ctx.n_head = n_head
        ctx.save_for_backward(qkv, out, lse)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        qkv, out, lse = ctx.saved_tensors
        B, T, C3 = qkv.shape
        H = ctx.n_head
        d = C3 // (3 * H)
        g = g.contiguous().float()
        dqkv = torch.empty_like(qkv)
        lib = _lib.load()
        with _lib.on_device(qkv.device):
            st = _lib.stream_ptr(qkv.device)
            nbytes = lib.spq_causal_attention_bwd_workspace_bytes(B, T, H, d)
            _lib.check(min(nbytes, 0), "spq_causal_attention_bwd_workspace_bytes")
            ws = _lib.workspace(qkv.device, nbytes, st)
            rc = lib.spq_causal_attention_bwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), g.data_ptr(), B, T, H, d,
                                              dqkv.data_ptr(), ws.data_ptr(), ws.numel(), st)
        _lib.check(rc, "spq_causal_attention_bwd")
        return dqkv, None


def causal_attention_autograd(qkv: torch.Tensor, n_head: int) -> torch.Tensor:
    """``causal_attention`` that records a gradient: the same forward launch (bit-identical ``out``), and
    ``spq_causal_attention_bwd`` hands back the gradient of ``qkv`` in ``qkv``'s own layout.  Head sizes ``BWD_HEAD_DIMS``; anything
    else raises (``served_backward`` tells beforehand).  Not twice differentiable.  When ``qkv`` needs no gradient, or gradients
    are disabled, this is ``causal_attention``."""
    if not (torch.is_grad_enabled() and qkv.requires_grad):
        return causal_attention(qkv, n_head)
    if qkv.dim() == 3 and qkv.shape[2] % (3 * n_head) == 0 and qkv.shape[2] // (3 * n_head) not in BWD_HEAD_DIMS:
        raise ValueError(f"causal_attention_autograd: head_dim {qkv.shape[2] // (3 * n_head)} has no backward kernel "
                         f"(served: {BWD_HEAD_DIMS})")
    return _CausalAttentionFunction.apply(qkv, n_head)
