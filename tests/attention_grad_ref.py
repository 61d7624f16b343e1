"""Reference gradients of the causal attention core and the bar they are judged by (shared by the attention-backward tests).

The reference is autograd through ``oracle.ref_cpu.attention_core`` on the CPU, in float64 (the yardstick) and in float32 (whose
own distance from float64, e_ref, widens the bar as in ``test_gpu_attention.judge``).  Each third of the gradient -- dq, dk, dv --
is judged on its own: bound = 1e-5 |y| + 1e-5 rms(y) with y that third in float64, the kernel is allowed (1 + e_ref) bounds, and
a third whose float64 reference is identically zero must come out exactly zero."""
import functools

import torch


def make_case(B, T, H, d, scale=1.0, offset=0.0, seed=0):
    """(qkv [B, T, 3 H d], dout [B, T, H d]) on the CPU, fp32"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3 * H * d, generator=g) * scale + offset
    dout = torch.randn(B, T, H * d, generator=g)
    return qkv, dout


def ref_grad(qkv_cpu, dout_cpu, n_head, dtype):
    """d(sum(attention_core(qkv) * dout)) / d qkv by CPU autograd in ``dtype``"""
    from oracle import ref_cpu as O
    x = qkv_cpu.to(dtype).clone().requires_grad_(True)
    out = O.attention_core(x, n_head)
    out.backward(dout_cpu.to(dtype))
    return x.grad.detach()


@functools.lru_cache(maxsize=None)
def cached_case(B, T, H, d, scale=1.0, offset=0.0, seed=0):
    """(qkv, dout, grad64, grad32) of ``make_case``: computed once, shared among the tests, never modified"""
    qkv, dout = make_case(B, T, H, d, scale, offset, seed)
    return qkv, dout, ref_grad(qkv, dout, H, torch.float64), ref_grad(qkv, dout, H, torch.float32)


def judge_tensor(got, ref32, ref64, what, standard=True, check=True):
    """err/bound of ``got`` and of the fp32 reference against float64 under 1e-5 |y| + 1e-5 rms(y); asserts e <= 1 + e_ref"""
    y = ref64.double()
    g = got.detach().cpu().double()
    if not bool(y.any()):
        print(f"[attention bwd] {what}: float64 reference identically zero")
        if check:
            assert not bool(g.any()), f"{what}: reference identically zero, got max |x| = {float(g.abs().max()):.3e}"
        return 0.0, 0.0
    bound = 1e-5 * y.abs() + 1e-5 * float(y.pow(2).mean().sqrt())
    e_ref = float(((ref32.detach().cpu().double() - y).abs() / bound).max())
    e = float(((g - y).abs() / bound).max())
    print(f"[attention bwd] {what}: kernel err/bound {e:.3f}, fp32 autograd err/bound {e_ref:.3f}, allowed {1 + e_ref:.3f}")
    if check:
        if standard:
            assert e_ref <= 1.0, f"{what}: not a standard case, the fp32 reference itself is at {e_ref:.3f}"
        assert e <= 1.0 + e_ref, f"{what}: err/bound {e:.3f} > 1 + e_ref = {1 + e_ref:.3f}"
    return e, e_ref


def judge_thirds(got, ref32, ref64, what, standard=True, check=True):
    """``judge_tensor`` on dq, dk and dv separately; ``got`` / refs are [B, T, 3C].  Returns {third: (e, e_ref)}"""
    C = ref64.shape[-1] // 3
    res = {}
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        res[name] = judge_tensor(got[..., sl], ref32[..., sl], ref64[..., sl], f"{what} {name}", standard, check)
    return res
