"""The causal attention core between c_attn and c_proj (models_sp.py:61-75) as one HIP launch: ``spq_causal_attention_fwd``
(csrc/spq_attention.hip).  Forward only; ``SPAttention.core`` uses it when ``use_hip_core`` is set."""
import torch

from . import _lib

HEAD_DIMS = (16, 32, 64, 80, 128)         # what spq_causal_attention_fwd serves; 64 is every GPT-2 size


def served(qkv: torch.Tensor, n_head: int) -> bool:
    """Can ``causal_attention`` take this tensor as it is (no copy, no cast)?"""
    return (qkv.is_cuda and qkv.dtype == torch.float32 and qkv.dim() == 3 and qkv.is_contiguous() and qkv.numel() > 0
            and qkv.shape[2] % (3 * n_head) == 0 and qkv.shape[2] // (3 * n_head) in HEAD_DIMS and qkv.data_ptr() % 16 == 0)


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
