"""Shared by the LM-loss tests: the yardstick (the reference's two loss lines, models_sp.py:443-449, under torch's CPU autograd in
float64 and in fp32), the project's bar, the input families and the judge.

Bar (as tests/ln_grad_ref.py): |got - ref| <= 1e-5 |ref| + 1e-5 rms(ref), applied separately to the per-row NLL, the
scalar loss and dlogits.  Every result is judged against float64; the allowed err/bound is 1 + e_ref, with e_ref the fp32 CPU
run's own err/bound against float64 (a result as far from the fp32 reference as the bar allows may be that much further from
float64, no more).  An element whose float64 value is exactly zero under a zero bound must be exactly zero."""
import functools

import torch
import torch.nn.functional as F

TOL = 1e-5
FAMILIES = ("randn", "randn_x3", "randn_x50", "randn_plus_1e4", "randn_x2.5_minus_30")
E_REF_LIMIT = 0.15            # what the fp32 reference stays under on every family at (B, T) = (2, 9) (test_lm_loss_host.py)


def bar_ratio(got, ref, tol=TOL):
    """max |got - ref| / (tol |ref| + tol rms(ref)); an element with a zero bound gives 0 when it is exactly equal and inf
    otherwise; a NaN anywhere gives NaN, so `<=` fails."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    rms = float(ref.pow(2).mean().sqrt())
    bound = tol * ref.abs() + tol * rms
    err = (got - ref).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def make_logits(family, B, T, V, seed):
    x = torch.randn(B, T, V, generator=torch.Generator().manual_seed(seed))
    if family == "randn_x3":
        x = x * 3.0
    elif family == "randn_x50":                              # near one-hot rows
        x = x * 50.0
    elif family == "randn_plus_1e4":
        x = x + 1e4
    elif family == "randn_x2.5_minus_30":
        x = x * 2.5 - 30.0
    else:
        assert family == "randn", family
    return x.contiguous()


def make_labels(B, T, V, seed):
    return torch.randint(V, (B, T), generator=torch.Generator().manual_seed(seed + 7919), dtype=torch.int64)


def reference(logits, labels, shift=True, ignore_index=-100, reduction="mean", upstream=None, dtype=torch.float64):
    """The reference's loss under CPU autograd in `dtype` -> dict(nll [B, T - shift], lse [B, T], sum, mean, out, dlogits).
    `upstream`: the gradient of `out` (default ones)."""
    x = logits.detach().cpu().to(dtype).clone().requires_grad_(True)
    lab = labels.detach().cpu()
    V = x.shape[-1]
    if shift:
        sl, ll = x[..., :-1, :].contiguous(), lab[..., 1:].contiguous()
    else:
        sl, ll = x, lab
    flat, flat_l = sl.view(-1, V), ll.view(-1)
    with torch.no_grad():
        nll = F.cross_entropy(flat, flat_l, ignore_index=ignore_index, reduction="none").view(ll.shape)
        total = F.cross_entropy(flat, flat_l, ignore_index=ignore_index, reduction="sum")
        count = int((flat_l != ignore_index).sum())
        mean = total / count if count else total * float("nan")
        lse = torch.logsumexp(x, dim=-1)
    if flat.shape[0] == 0:                                   # T = 1 under the shift: nothing is scored
        return dict(nll=nll, lse=lse, sum=total, mean=mean, out=None, dlogits=torch.zeros_like(x))
    out = F.cross_entropy(flat, flat_l, ignore_index=ignore_index, reduction=reduction)
    if reduction == "none":
        out = out.view(ll.shape)
    g = torch.ones_like(out) if upstream is None else upstream.detach().cpu().to(dtype).reshape(out.shape)
    if count or reduction != "mean":
        out.backward(g)
        dlogits = x.grad
    else:
        dlogits = torch.zeros_like(x)                        # mean over no row: torch's gradient is 0 * NaN; the kernel's is zeros
    return dict(nll=nll, lse=lse, sum=total, mean=mean, out=out.detach(), dlogits=dlogits)


def yardstick(logits, labels, **kw):
    """(float64 reference, e_ref per key): e_ref[k] is the fp32 CPU run's err/bound against float64."""
    r64 = reference(logits, labels, dtype=torch.float64, **kw)
    r32 = reference(logits, labels, dtype=torch.float32, **kw)
    e_ref = {k: bar_ratio(r32[k], r64[k]) for k in ("nll", "lse", "sum", "mean", "dlogits")
             if not bool(torch.isnan(r64[k]).any())}
    return r64, e_ref


@functools.lru_cache(maxsize=None)
def cached_case(family, B, T, V, shift, seed):
    """logits, labels and their yardstick (mean reduction, upstream 1), computed once and shared; treat them as read-only."""
    logits, labels = make_logits(family, B, T, V, seed), make_labels(B, T, V, seed)
    r64, e_ref = yardstick(logits, labels, shift=shift)
    return logits, labels, r64, e_ref


def judge(got, r64, e_ref, key, what):
    """Assert got within (1 + e_ref) of the bar against float64; returns (err/bound, e_ref) for the parity table."""
    ratio, allowed = bar_ratio(got, r64[key]), 1.0 + e_ref[key]
    print(f"[lm loss] {what} {key}: err/bound {ratio:.3f} (fp32 reference {e_ref[key]:.3f})")
    assert ratio <= allowed, f"{what} {key}: err/bound {ratio:.3f} > {allowed:.3f}"
    return ratio, e_ref[key]
