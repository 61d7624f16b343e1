"""Shared by the SwitchableLayerNorm autograd tests and their fixture generator: the yardstick (the oracle's formula under torch's
CPU autograd, fp32 and fp64), the project's gradient bar, the input distributions and the slab cut of the column sums."""
import torch

from oracle import ref_cpu as O

TOL = 1e-5            # |d| <= 1e-5 |ref| + 1e-5 rms(ref)
FP32_REF_LIMIT = 0.25  # the fp32 reference is the yardstick only where it is itself within a quarter of the bar of fp64


def bar_ratio(got, ref, tol=TOL):
    """max |got - ref| / (tol |ref| + tol rms(ref)) over every element (NaN if anything is NaN, so `<=` fails)."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    rms = float(ref.pow(2).mean().sqrt())
    bound = tol * ref.abs() + tol * rms
    r = (got - ref).abs() / bound
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def oracle_grads(x, g, weight, bias, eps=1e-5, dtype=torch.float32):
    """(y, dx, dweight, dbias) of oracle.ref_cpu.switchable_layernorm under torch's CPU autograd in `dtype`."""
    xs, ws, bs = (t.detach().cpu().to(dtype).clone().requires_grad_(True) for t in (x, weight, bias))
    y = O.switchable_layernorm(xs, ws, bs, eps)
    y.backward(g.detach().cpu().to(dtype))
    return y.detach(), xs.grad, ws.grad, bs.grad


def yardstick(x, g, weight, bias, eps=1e-5):
    """The reference gradients a case is judged against and the allowed err/bound.

    The fp32 autograd of the reference's formula is the yardstick where it is itself well inside the bar against the same formula
    in fp64 (err/bound <= 0.25).  Where it is not (rows with a large common offset: x - mean cancels), the case is judged against
    fp64, and the allowance is 1 + the fp32 reference's own err/bound: a result as far from the fp32 reference as the bar allows may
    be that much further from fp64 (triangle inequality), no more.  Returns (dx, dweight, dbias), limit, ref_ratio, name."""
    _, *r32 = oracle_grads(x, g, weight, bias, eps, torch.float32)
    _, *r64 = oracle_grads(x, g, weight, bias, eps, torch.float64)
    ratio = max(bar_ratio(a, b) for a, b in zip(r32, r64))
    if ratio <= FP32_REF_LIMIT:
        return r32, 1.0, ratio, "fp32"
    return r64, 1.0 + ratio, ratio, "fp64"


DISTRIBUTIONS = ("normal", "outliers", "heavy", "channel", "tiny")


def make_input(dist, rows, cols, seed):
    """The five input distributions of tools/fuzz_parity.py, restated on a seeded generator."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, cols, generator=gen)
    if dist == "outliers":                                   # 1 % of the elements twenty times larger
        x = torch.where(torch.rand(rows, cols, generator=gen) < 0.01, x * 20.0, x)
    elif dist == "heavy":                                    # Student t, 3 degrees of freedom
        chi2 = torch.randn(3, rows, cols, generator=gen).pow(2).sum(0)
        x = x / torch.sqrt(chi2 / 3.0)
    elif dist == "channel":                                  # one hot channel
        x[:, int(torch.randint(cols, (1,), generator=gen))] *= 60.0
    elif dist == "tiny":
        x = x * 1e-6
    else:
        assert dist == "normal", dist
    return x.contiguous()


def make_case(dist, rows, cols, seed):
    """x, g, weight, bias of one seeded case."""
    x = make_input(dist, rows, cols, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    g = torch.randn(rows, cols, generator=gen)
    weight = torch.randn(cols, generator=gen) * 0.2 + 1.0
    bias = torch.randn(cols, generator=gen) * 0.1
    return x, g, weight, bias


# the slab cut of spq_layernorm_bwd's column sums (include/spq.h): a function of rows only
MAX_SLABS, MIN_SLAB_ROWS = 512, 16


def slabs(rows):
    return min(MAX_SLABS, -(-rows // MIN_SLAB_ROWS))


def slab_range(rows, s):
    """rows [first, last) of slab s: sizes differ by one at most"""
    S = slabs(rows)
    return s * rows // S, (s + 1) * rows // S
