"""Float64 closed form of the two linear layers' backward (``_SPLinearFunction.backward`` in sp_linear.py,
``_CPTLinearFunction.backward`` in cpt.py), the case tables of the contraction-kernel edge tests, and the input recipe
that makes every gradient clamp fire.  Test infrastructure: nothing here runs a kernel.

The closed forms take operands that are ALREADY fake-quantised -- FQ(W), FQ(A), FQ(B), FQ(x) as the product's own
quantisers produced them -- and quantise nothing, so a level that flips at a rounding tie never enters a contraction
test (the quantisers have their own tests).  The straight-through estimators are the reference's: identity for a
min-max quantiser, ``clamp(grad, -10, 10)`` for a log quantiser.

The two layers differ in where the input clamp sits, and the two functions encode exactly that:

    SP   (part 1: the LoRA branch reads the RAW x)      gx = clamp(g . FQ(W)) + s (g . FQ(B)^T) . FQ(A)^T
    CPT  (part 2: the LoRA branch reads FQ(x))          gx = clamp(g . (FQ(W) + s FQ(B) FQ(A)^T))

Every clamped output comes with its pre-clamp value under ``pre_*``; the tests take their error bound at that scale
(``worst_ratio``): clamping is 1-Lipschitz, so an error bound on the argument carries over to the result, while a bound
at the scale of the clamped result does not hold for any fp32 implementation once most elements sit at +-10.
"""
import math

import torch

CLAMP = 10.0


def _d(t):
    return None if t is None else t.detach().double()


def _clamp(t, on):
    return t.clamp(-CLAMP, CLAMP) if on else t


def sp_backward(g, wq, x, xq=None, aq=None, bq=None, s=0.0, log_x=False, log_w=False, log_a=False, log_b=False):
    """SPLinearWithLoRA.  g [M, N], wq = FQ(W) [N, K], x raw [M, K], xq = FQ(x) [M, K] (d/dW only), aq = FQ(A) [K, r],
    bq = FQ(B) [r, N], s = alpha / rank; aq = None: no adapter.  ``log_*``: that quantiser is a log quantiser.  Returns a dict
    of float64 tensors: gx, gA, gB, gW, gb, t (= x . FQ(A), what the forward saves for d/dB), pre_base (= g . FQ(W), the
    clamped term of gx), lora (the unclamped term of gx), pre_gx (= |pre_base| + |lora|, the scale of gx's bound), pre_gA,
    pre_gB, pre_gW."""
    g, wq, x, xq, aq, bq = (_d(v) for v in (g, wq, x, xq, aq, bq))
    out = {"pre_base": g @ wq, "gb": g.sum(dim=0)}
    out["lora"] = torch.zeros_like(out["pre_base"])
    if aq is not None:
        gt = g @ bq.t()                                         # [M, r]
        out["lora"] = s * (gt @ aq.t())
        out["t"] = x @ aq
        out["pre_gA"] = s * (x.t() @ gt)
        out["pre_gB"] = s * (out["t"].t() @ g)
        out["gA"] = _clamp(out["pre_gA"], log_a)
        out["gB"] = _clamp(out["pre_gB"], log_b)
    out["gx"] = _clamp(out["pre_base"], log_x) + out["lora"]
    out["pre_gx"] = out["pre_base"].abs() + out["lora"].abs()
    if xq is not None:
        out["pre_gW"] = g.t() @ xq
        out["gW"] = _clamp(out["pre_gW"], log_w)
    return out


def sp_backward_wrong_order(g, wq, aq, bq, s):
    """The mistake the active-clamp inputs are there to catch: clamp(base + lora) instead of clamp(base) + lora."""
    g, wq, aq, bq = (_d(v) for v in (g, wq, aq, bq))
    return (g @ wq + s * ((g @ bq.t()) @ aq.t())).clamp(-CLAMP, CLAMP)


def cpt_backward(g, wq, xq, aq=None, bq=None, s=0.0, log_in=False, log_w=False, log_l=False):
    """CPTLinear with its gradient quantisers off.  g [M, N], wq [N, K], xq = FQ(x) [M, K], aq = FQ(A) [K, r],
    bq = FQ(B) [N, r].  Returns gx, gA, gB, gW, gb, t (= FQ(x) . FQ(A)) and pre_gx (= g . W_eff, clamped WHOLE), pre_gA,
    pre_gB, pre_gW."""
    g, wq, xq, aq, bq = (_d(v) for v in (g, wq, xq, aq, bq))
    w_eff = wq if aq is None else wq + s * (bq @ aq.t())
    out = {"pre_gx": g @ w_eff, "gb": g.sum(dim=0), "pre_gW": g.t() @ xq}
    out["gx"] = _clamp(out["pre_gx"], log_in)
    out["gW"] = _clamp(out["pre_gW"], log_w)
    if aq is not None:
        out["t"] = xq @ aq
        out["pre_gA"] = s * (xq.t() @ (g @ bq))
        out["pre_gB"] = s * (g.t() @ out["t"])
        out["gA"] = _clamp(out["pre_gA"], log_l)
        out["gB"] = _clamp(out["pre_gB"], log_l)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The bar: |d| <= 1e-5 |pre| + 1e-5 rms(pre).  With pre = the reference itself this is helpers.assert_close_y.
# ---------------------------------------------------------------------------------------------------------------------
def worst_ratio(got, ref, pre=None, rel=1e-5):
    """max |got - ref| / (rel |pre| + rel rms(pre)); pre defaults to ref."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    pre = ref if pre is None else pre.detach().double().cpu().reshape(ref.shape)
    bound = rel * pre.abs() + rel * float(pre.pow(2).mean().sqrt())
    return float(((got - ref).abs() / bound).max())


def share_outside(pre):
    """fraction of elements a clamp to +-10 changes"""
    return float((pre.abs() > CLAMP).double().mean())


def std_of(t):
    t = t.detach().double()
    return float(t.pow(2).mean().sqrt()) if t.numel() == 1 else float(t.std())


def make_inputs(M, K, N, r, seed, b_nr=False):
    """W, bias, A, B (random, not the zero initialisation; [N, r] with ``b_nr``), x, a second activation batch for calibration,
    and an incoming gradient g, all fp32 on the CPU.  The weights are the synthetic workload's; x is plain N(0, 1) WITHOUT that
    workload's x20 outlier entries: at rank 1, d/dA has K elements, and a single outlier product would carry their whole standard
    deviation (measured: one element at 84 with the other 95 below 15), which is not what "standard deviation 10" is meant to set."""
    from llm_qat_on_gpt2_amd.synthetic import make_workload
    W, bias, A, B, _, _ = make_workload(max(M, 2), K, N, r, seed=seed)
    gen = torch.Generator().manual_seed(7000 + seed)
    x, x_cal, g = torch.randn(M, K, generator=gen), torch.randn(M, K, generator=gen), torch.randn(M, N, generator=gen)
    return W, bias, A, (B.t().contiguous() if b_nr else B), x, x_cal, g


# ---------------------------------------------------------------------------------------------------------------------
# Inputs under which every clamp is active, scaled from the reference alone.  The callers supply the quantisers
# (the GPU tests the product's, the CPU test the oracle's) as callables that RECALIBRATE on what they are given.
# ---------------------------------------------------------------------------------------------------------------------
def sp_clamp_inputs(g, x, B, wq, aq, s, fq_b):
    """g, then x, then B, each a scalar multiple of what came in, such that g . FQ(W), pre-clamp gB and pre-clamp gA have
    standard deviation 10.  gx does not depend on x and gB does not depend on B, so no step undoes an earlier one.
    ``fq_b(B)`` -> FQ(B) [r, N] with B's quantiser recalibrated on B."""
    g = g * (CLAMP / std_of(_d(g) @ _d(wq)))
    x = x * (CLAMP / std_of(s * ((_d(x) @ _d(aq)).t() @ _d(g))))
    B = B * (CLAMP / std_of(s * (_d(x).t() @ (_d(g) @ _d(fq_b(B)).t()))))
    return g, x, B


def cpt_clamp_inputs(g, x, B, wq, s, fq_l, fq_x):
    """The same for CPTLinear, where the adapter is folded into the clamped product g . W_eff, so g's scale depends on B's:
    B first (the ratio std(gB) / std(gA) does not depend on the scales of g and x), then g, then x.  ``fq_l(B)`` -> (FQ(A)
    [K, r], FQ(B) [N, r]) with the shared adapter quantiser recalibrated on A then B; ``fq_x(x)`` -> FQ(x) with the input
    quantiser recalibrated on x."""
    aq, bq = (_d(v) for v in fq_l(B))
    xq = _d(fq_x(x))
    B = B * (std_of(s * (_d(g).t() @ (xq @ aq))) / std_of(s * (xq.t() @ (_d(g) @ bq))))
    aq, bq = (_d(v) for v in fq_l(B))
    g = g * (CLAMP / std_of(_d(g) @ (_d(wq) + s * (bq @ aq.t()))))
    x = x * (CLAMP / std_of(s * (_d(g).t() @ (xq @ aq))))
    return g, x, B


# ---------------------------------------------------------------------------------------------------------------------
# Case tables.  Shapes of the layer tests: (M, K, N, r).
# ---------------------------------------------------------------------------------------------------------------------
SP_SHAPES = [(37, 100, 72, 5), (129, 96, 132, 16), (200, 260, 200, 63), (300, 64, 520, 129), (64, 96, 128, 1), (1, 96, 128, 16)]
SP_CLAMP_SHAPES = SP_SHAPES[:5]
CPT_SHAPES = SP_SHAPES[:3]
# _LimbGemm: (M, C, R, r)
LIMB_SHAPES = [(1, 8, 4, 1), (37, 72, 100, 5), (129, 132, 96, 16), (200, 200, 260, 63), (300, 520, 64, 64), (300, 520, 64, 65),
               (257, 260, 200, 128), (130, 99, 50, 7)]


def ld_above(n, mod, res):
    """smallest leading dimension > n with ld % mod == res"""
    ld = n + 1
    while ld % mod != res:
        ld += 1
    return ld


# spq_gemm_f32_tn.  Shapes (M, I, J); the planner's (S, rows per slice) of each is asserted in test_linear_grad_ref_cpu.py from
# the library's own workspace function.
TN_SHAPES = [(1, 1, 1), (15, 3, 5), (65, 64, 128), (129, 16, 132), (257, 66, 128), (385, 65, 7), (513, 2, 260), (641, 16, 64),
             (1000, 200, 520), (2305, 130, 130), (4096, 256, 1024), (16385, 8, 8),
             (67, 63, 127), (13, 130, 3)]                       # the I and J tile edges the planner rows above leave out
TN_EXPECTED_PLAN = {(1, 1, 1): (1, 16), (15, 3, 5): (1, 16), (65, 64, 128): (1, 80), (129, 16, 132): (2, 80), (257, 66, 128): (3, 96),
                    (385, 65, 7): (4, 112), (513, 2, 260): (5, 112), (641, 16, 64): (6, 112), (1000, 200, 520): (8, 128),
                    (2305, 130, 130): (19, 128), (4096, 256, 1024): (16, 256), (16385, 8, 8): (128, 144)}
# layouts: (ldp rule, ldq rule, P offset in floats, Q offset in floats); a rule is None (= the row length) or (mod, residue)
TN_LAYOUTS = {
    "dense":        (None,   None,   0, 0),      # both vector paths wherever the row length and the tile allow
    "padded_vec":   ((2, 0), (4, 0), 0, 0),      # ld > row, still even / a multiple of 4: vector loads with a pitch
    "odd_ld":       ((2, 1), (4, 1), 0, 0),      # odd ldp, ldq % 4 == 1: scalar loads of both operands
    "ldq2_p_off":   ((2, 0), (4, 2), 1, 0),      # ldq % 4 == 2; P one float past a 16-byte boundary
    "q_off":        ((2, 0), (4, 0), 0, 1),      # aligned pitches, Q one float past a 16-byte boundary
}
TN_ALPHAS = (1.0, 0.5, -2.0)


def tn_cases():
    """(M, I, J, layout name, alpha): every shape in every layout, the three alphas dealt round robin"""
    out = []
    for si, shape in enumerate(TN_SHAPES):
        for li, name in enumerate(TN_LAYOUTS):
            out.append(shape + (name, TN_ALPHAS[(si + li) % 3]))
    return out


def tn_leading_dims(I, J, layout):
    rp, rq, offp, offq = TN_LAYOUTS[layout]
    return (I if rp is None else ld_above(I, *rp)), (J if rq is None else ld_above(J, *rq)), offp, offq


def tn_plan(lib, M, I, J):
    """(S, rows per slice) as the library will run it, derived from its own workspace function: no mirror of the planner"""
    extra = lib.spq_gemm_f32_tn_workspace_bytes(M, I, J) - 256
    S = extra // (4 * I * J) if extra > 0 else 1
    return S, (math.ceil(math.ceil(M / S) / 16)) * 16


# spq_gemm_f32_nt.  A case is a dict: M, N, K, lda, ldb, offa, offb, K2, lda2, ldb2, offa2, offb2, alpha2, bias.
def _pad4(k):
    return (k + 3) // 4 * 4


def _odd_at_least(k):
    return k if k % 2 else k + 1


NT_MN = (1, 127, 128, 129, 257)
NT_KS = (1, 3, 31, 32, 33, 35, 64, 100)
NT_K2S = (0, 1, 16, 33, 129)
NT_WG_SHAPES = {1: (5, 9), 7: (5, 893), 8: (1000, 9), 9: (300, 300), 12: (300, 500), 15: (600, 300), 17: (2100, 9)}   # tiles_m * tiles_n -> (M, N)


def nt_case(M, N, K, lda=None, ldb=None, offa=0, offb=0, K2=0, lda2=None, ldb2=None, offa2=0, offb2=0, alpha2=1.0, bias=True,
            tag=""):
    return dict(M=M, N=N, K=K, lda=lda or K, ldb=ldb or K, offa=offa, offb=offb, K2=K2, lda2=lda2 or max(K2, 1),
                ldb2=ldb2 or max(K2, 1), offa2=offa2, offb2=offb2, alpha2=alpha2, bias=bias, tag=tag)


def nt_fast(c):
    """which instantiation the library's dispatch takes (spq_gemm_f32.hip launch_gemm_f32_nt): the vector-load one needs every
    operand 16-byte aligned with a pitch that is a multiple of 4 floats.  Base buffers are 16-byte aligned, so an operand is
    aligned iff its offset is a multiple of 4 floats."""
    ok = c["offa"] % 4 == 0 and c["offb"] % 4 == 0 and c["lda"] % 4 == 0 and c["ldb"] % 4 == 0
    if c["K2"] > 0:
        ok = ok and c["offa2"] % 4 == 0 and c["offb2"] % 4 == 0 and c["lda2"] % 4 == 0 and c["ldb2"] % 4 == 0
    return ok


def nt_cases():
    out = []
    i = 0
    for K in NT_KS:                                               # the K edges in both instantiations
        for tag, kw in (("tight", dict()),
                        ("pad4", dict(lda=_pad4(K), ldb=_pad4(K))),                            # FAST, with its K tail when K % 4 != 0
                        ("odd_ldb", dict(lda=_pad4(K), ldb=_odd_at_least(K + 1))),             # scalar loads forced by the pitch
                        ("a_off", dict(lda=_pad4(K), ldb=_pad4(K), offa=1))):                  # ... and by the base pointer
            M, N = NT_MN[i % 5], NT_MN[(2 * i + i // 5) % 5]
            out.append(nt_case(M, N, K, alpha2=1.0, bias=(i % 2 == 0), tag=f"K{K}_{tag}", **kw))
            i += 1
    for j, K2 in enumerate(NT_K2S):                               # the second segment
        for tag, kw in (("pad4", dict(lda2=_pad4(K2), ldb2=_pad4(K2))), ("tight", dict())):
            if K2 == 0 and tag == "tight":
                continue
            out.append(nt_case(129, 127, 33, lda=36, ldb=36, K2=K2, alpha2=(0.5, 1.0)[(j + (tag == "tight")) % 2], bias=(j % 2 == 1),
                               tag=f"K2_{K2}_{tag}", **kw))
    out.append(nt_case(129, 127, 32, K2=16, offa2=1, alpha2=0.5, bias=True, tag="only_A2_misaligned"))
    out.append(nt_case(257, 257, 64, K2=16, alpha2=0.5, bias=False, tag="257x257_two_segments"))
    for nwg, (M, N) in NT_WG_SHAPES.items():                      # the XCD remap of the workgroup index
        out.append(nt_case(M, N, 8, K2=(4 if nwg % 2 else 0), alpha2=0.5, bias=(nwg % 3 == 0), tag=f"wg{nwg}"))
    return out
