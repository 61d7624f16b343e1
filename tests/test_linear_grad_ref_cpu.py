"""No GPU: the float64 closed forms of tests/linear_grad_ref.py against torch autograd on a plain-torch model of the same
straight-through estimators, the clamp-activating input recipe on the reference alone, and the coverage the case tables of
the contraction edge tests claim -- the token contraction's from the library's own host function (needs the built library,
no device, as test_split_k_host.py does)."""
import math

import pytest
import torch

import linear_grad_ref as R


class _FQ(torch.autograd.Function):
    """A toy quantiser (round to eighths) with the reference's straight-through backward: identity (min-max) or
    clamp(grad, -10, 10) (log)."""

    @staticmethod
    def forward(ctx, t, log):
        ctx.log = log
        return torch.round(t * 8) / 8

    @staticmethod
    def backward(ctx, grad):
        return (grad.clamp(-10, 10) if ctx.log else grad), None


def _leaves(M, K, N, r, seed, b_nr=False):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, W, bias, A = mk(M, K), mk(N, K), mk(N), mk(K, r)
    B = mk(N, r) if b_nr else mk(r, N)
    gy = mk(M, N) * 30.0                                         # large enough that every clamp changes something
    return [t.requires_grad_(True) for t in (x, W, bias, A, B)], gy


FLAG_SETS = [(False, False, False, False), (True, True, True, True), (True, False, False, True), (False, True, True, False)]


@pytest.mark.parametrize("shape", [(7, 5, 6, 3), (1, 5, 6, 3), (7, 5, 6, 1), (1, 4, 3, 1)])
@pytest.mark.parametrize("flags", FLAG_SETS)
def test_sp_closed_form_is_what_autograd_gives(shape, flags):
    M, K, N, r = shape
    log_x, log_w, log_a, log_b = flags
    (x, W, bias, A, B), gy = _leaves(M, K, N, r, seed=M + 10 * r)
    s = 1.5
    y = _FQ.apply(x, log_x) @ _FQ.apply(W, log_w).t() + bias + s * ((x @ _FQ.apply(A, log_a)) @ _FQ.apply(B, log_b))
    y.backward(gy)
    fq = lambda t: (torch.round(t * 8) / 8).detach()
    ref = R.sp_backward(gy, fq(W), x, fq(x), fq(A), fq(B), s, log_x, log_w, log_a, log_b)
    for name, leaf in (("gx", x), ("gW", W), ("gb", bias), ("gA", A), ("gB", B)):
        assert torch.allclose(ref[name], leaf.grad, rtol=1e-12, atol=1e-12), name
    if all(flags):
        for name in ("pre_base", "pre_gA", "pre_gB", "pre_gW"):
            assert R.share_outside(ref[name]) > 0, f"{name}: the clamp changed nothing, the comparison above proves nothing"
        wrong = R.sp_backward_wrong_order(gy, fq(W), fq(A), fq(B), s)
        assert not torch.allclose(wrong, x.grad)
    assert torch.equal(ref["t"], (x @ fq(A)).detach())
    # without an adapter
    (x, W, bias, _, _), gy = _leaves(M, K, N, r, seed=M + 10 * r)
    (_FQ.apply(x, log_x) @ _FQ.apply(W, log_w).t() + bias).backward(gy)
    ref = R.sp_backward(gy, fq(W), x, fq(x), log_x=log_x, log_w=log_w)
    assert torch.allclose(ref["gx"], x.grad, rtol=1e-12, atol=1e-12) and torch.allclose(ref["gW"], W.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", [(7, 5, 6, 3), (1, 5, 6, 3), (7, 5, 6, 1), (1, 4, 3, 1)])
@pytest.mark.parametrize("flags", [(False, False, False), (True, True, True), (True, False, False), (False, False, True)])
def test_cpt_closed_form_is_what_autograd_gives(shape, flags):
    M, K, N, r = shape
    log_in, log_w, log_l = flags
    (x, W, bias, A, B), gy = _leaves(M, K, N, r, seed=3 + M + 10 * r, b_nr=True)
    s = 2.0
    xq = _FQ.apply(x, log_in)
    y = xq @ _FQ.apply(W, log_w).t() + bias + s * ((xq @ _FQ.apply(A, log_l)) @ _FQ.apply(B, log_l).t())
    y.backward(gy)
    fq = lambda t: (torch.round(t * 8) / 8).detach()
    ref = R.cpt_backward(gy, fq(W), fq(x), fq(A), fq(B), s, log_in, log_w, log_l)
    for name, leaf in (("gx", x), ("gW", W), ("gb", bias), ("gA", A), ("gB", B)):
        assert torch.allclose(ref[name], leaf.grad, rtol=1e-12, atol=1e-12), name
    if all(flags):
        for name in ("pre_gx", "pre_gA", "pre_gB", "pre_gW"):
            assert R.share_outside(ref[name]) > 0, name
    assert torch.equal(ref["t"], (fq(x) @ fq(A)).detach())


def test_the_two_layers_differ_exactly_in_where_the_input_clamp_sits():
    """same operands (B transposed): SP clamps g . FQ(W) and adds the adapter term, CPT clamps the sum"""
    (x, W, bias, A, B), gy = _leaves(9, 6, 7, 2, seed=11)
    sp = R.sp_backward(gy, W, x, x, A, B, 1.0, log_x=True)
    cpt = R.cpt_backward(gy, W, x, A, B.t(), 1.0, log_in=True)
    assert torch.allclose(sp["pre_base"] + sp["lora"], cpt["pre_gx"], rtol=1e-12, atol=1e-12)
    assert torch.equal(cpt["gx"], cpt["pre_gx"].clamp(-10, 10))
    assert torch.equal(sp["gx"], sp["pre_base"].clamp(-10, 10) + sp["lora"])
    assert torch.allclose(R.sp_backward_wrong_order(gy, W, A, B, 1.0), cpt["gx"], rtol=1e-12, atol=1e-12)
    assert not torch.allclose(sp["gx"], cpt["gx"])


# ---------------------------------------------------------------------------------------------------------------------
# The active-clamp input recipe, on the reference alone (6-bit log, per channel: the oracle's quantisers stand in for the product's)
# ---------------------------------------------------------------------------------------------------------------------
def _shares_ok(ref, names, what):
    for name in names:
        sh = R.share_outside(ref[name])
        assert 0.10 <= sh <= 0.60, f"{what}: {sh:.3f} of {name} lies outside +-10"


@pytest.mark.parametrize("shape", R.SP_CLAMP_SHAPES)
def test_sp_clamp_recipe(shape):
    from oracle import ref_cpu as O
    M, K, N, r = shape
    W, bias, A, B, x0, x1, g = R.make_inputs(M, K, N, r, seed=5)
    ol = O.build_calibrated_layer(W, bias, A, B, [x0, x1], 6, "log", True, 2.0 * r, r)
    s = ol.scaling
    wq, aq = ol.qw(W), ol.qA(A)
    fq_b = lambda b: O.QuantState(6, "log", 1, True).calibrate_on(b)(b)
    g, x, B = R.sp_clamp_inputs(g, x0, B, wq, aq, s, fq_b)
    assert g.dtype == x.dtype == B.dtype == torch.float32
    bq = fq_b(B)
    xq = O.QuantState(6, "log", -1, True).calibrate_on(x)(x)
    ref = R.sp_backward(g, wq, x, xq, aq, bq, s, True, True, True, True)
    _shares_ok(ref, ("pre_base", "pre_gA", "pre_gB"), f"SP {shape}")
    # clamp(base + lora) must be far from clamp(base) + lora, in units of the bound the GPU test applies to gx
    wrong = R.sp_backward_wrong_order(g, wq, aq, bq, s)
    bound = 1e-5 * ref["pre_gx"] + 1e-5 * float(ref["pre_gx"].pow(2).mean().sqrt())
    far = float(((wrong - ref["gx"]).abs() > bound).double().mean())
    print(f"SP {shape}: shares base {R.share_outside(ref['pre_base']):.3f} gA {R.share_outside(ref['pre_gA']):.3f} "
          f"gB {R.share_outside(ref['pre_gB']):.3f}; wrong-order share {far:.3f}")
    assert far >= 0.20, f"SP {shape}: the wrong clamp order differs on only {far:.3f} of gx"
    # the bar is one an fp32 implementation can meet: the same closed form in fp32 on the CPU
    f = lambda t: t.float()
    gx32 = (f(g) @ f(wq)).clamp(-10, 10) + s * ((f(g) @ f(bq).t()) @ f(aq).t())
    gA32 = (s * (f(x).t() @ (f(g) @ f(bq).t()))).clamp(-10, 10)
    gB32 = (s * ((f(x) @ f(aq)).t() @ f(g))).clamp(-10, 10)
    for name, got, pre in (("gx", gx32, "pre_gx"), ("gA", gA32, "pre_gA"), ("gB", gB32, "pre_gB")):
        w = R.worst_ratio(got, ref[name], ref[pre])
        print(f"   fp32 CPU {name}: err/bound {w:.3f}")
        assert w <= 1.0, (name, w)


@pytest.mark.parametrize("shape", R.CPT_SHAPES)
def test_cpt_clamp_recipe(shape):
    from oracle import ref_cpt as C
    M, K, N, r = shape
    W, bias, A, B, x0, x1, g = R.make_inputs(M, K, N, r, seed=5, b_nr=True)
    s = 2.0

    def cal(cd, *ts):
        q = C.CPTQuantState(6, "log", cd, True)
        q.start()
        for t in ts:
            q(t)
        q.finish()
        return q
    wq = cal(0, W)(W)
    fq_l = lambda b: (lambda q: (q(A), q(b)))(cal(1, A, b))
    fq_x = lambda x: cal(-1, x)(x)
    g, x, B = R.cpt_clamp_inputs(g, x0, B, wq, s, fq_l, fq_x)
    aq, bq = fq_l(B)
    ref = R.cpt_backward(g, wq, fq_x(x), aq, bq, s, True, True, True)
    print(f"CPT {shape}: shares gx {R.share_outside(ref['pre_gx']):.3f} gA {R.share_outside(ref['pre_gA']):.3f} "
          f"gB {R.share_outside(ref['pre_gB']):.3f}")
    _shares_ok(ref, ("pre_gx", "pre_gA", "pre_gB"), f"CPT {shape}")


# ---------------------------------------------------------------------------------------------------------------------
# Case tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import llm_qat_on_gpt2_amd as p
    return p._lib.load()


def test_tn_table_reaches_every_launch_edge_of_the_planner(lib):
    plans = {s: R.tn_plan(lib, *s) for s in R.TN_SHAPES}
    for shape, want in R.TN_EXPECTED_PLAN.items():
        assert plans[shape] == want, (shape, plans[shape], want)
    S = {p[0] for p in plans.values()}
    assert 1 in S and 128 in S
    assert {(s - 1) % 4 for s in S if s > 1} == {0, 1, 2, 3}                    # the reduce kernel's unroll tail
    empty = {sh: sum(1 for s in range(S_) if s * rps >= sh[0]) for sh, (S_, rps) in plans.items()}   # slices with no token at all
    assert empty[(16385, 8, 8)] == 14
    batches = {math.ceil(rps / 64) for _, rps in plans.values()}                # the double-buffered loop's two exits
    assert any(b % 2 == 0 for b in batches) and any(b % 2 == 1 for b in batches) and max(batches) >= 3
    tiles = lambda sh: math.ceil(sh[1] / 64) * math.ceil(sh[2] / 128)
    assert any(S_ == 512 // tiles(sh) and S_ < math.ceil(sh[0] / 128) for sh, (S_, _) in plans.items())   # S limited by the tile count
    assert {1, 2, 63, 64, 65, 66, 130} <= {sh[1] for sh in R.TN_SHAPES}
    assert {1, 3, 127, 128, 132, 260} <= {sh[2] for sh in R.TN_SHAPES}
    Ms = [sh[0] for sh in R.TN_SHAPES]
    assert any(m % 2 for m in Ms) and any(m < 16 for m in Ms) and any(m % 64 == 1 and m > 64 for m in Ms)
    assert max(sh[0] * max(sh[1], sh[2]) for sh in R.TN_SHAPES) <= 4096 * 1024
    # layouts
    seen_p, seen_q = set(), set()
    for M, I, J, layout, alpha in R.tn_cases():
        ldp, ldq, offp, offq = R.tn_leading_dims(I, J, layout)
        assert ldp >= I and ldq >= J
        seen_p.add((ldp == I, ldp % 2, offp)); seen_q.add((ldq == J, ldq % 4, offq))
    assert {(False, 0, 0), (False, 1, 0), (False, 0, 1)} <= seen_p and any(t[0] for t in seen_p)
    assert {(False, 0, 0), (False, 1, 0), (False, 2, 0), (False, 0, 1)} <= seen_q and any(t[0] for t in seen_q)
    assert {c[4] for c in R.tn_cases()} == {1.0, 0.5, -2.0}
    # every shape with S > 1 meets an alpha other than 1 (the reduce kernel applies it, the tile kernel must not)
    for sh, (S_, _) in plans.items():
        assert S_ == 1 or any(c[4] != 1.0 for c in R.tn_cases() if c[:3] == sh)


def test_nt_table_reaches_every_branch_of_the_kernel():
    cases = R.nt_cases()
    assert len({c["tag"] for c in cases}) == len(cases)
    for c in cases:
        assert c["K"] <= 1024 and c["lda"] >= c["K"] and c["ldb"] >= c["K"] and c["alpha2"] in (1.0, 0.5)
        assert c["K2"] == 0 or (c["lda2"] >= c["K2"] and c["ldb2"] >= c["K2"])
    kc = [c for c in cases if c["tag"].startswith("K") and not c["tag"].startswith("K2")]
    for K in R.NT_KS:
        mine = [c for c in kc if c["K"] == K]
        assert any(R.nt_fast(c) for c in mine), K                                      # the vector-load instantiation ...
        assert any(R.nt_fast(c) and c["lda"] == R._pad4(K) for c in mine), K           # ... on its K tail whenever K % 4 != 0
        assert any(not R.nt_fast(c) and c["ldb"] % 2 == 1 and c["offa"] == 0 for c in mine), K     # scalar loads by an odd pitch
        assert any(not R.nt_fast(c) and c["ldb"] % 4 == 0 and c["lda"] % 4 == 0 and c["offa"] == 1 for c in mine), K   # by the pointer
        assert any(c["lda"] == K and c["ldb"] == K for c in mine), K
    assert {c["M"] for c in kc} >= set(R.NT_MN) and {c["N"] for c in kc} >= set(R.NT_MN)
    assert {c["K2"] for c in cases} >= set(R.NT_K2S)
    assert any(c["K2"] > 0 and c["alpha2"] == 1.0 for c in cases) and any(c["K2"] > 0 and c["alpha2"] == 0.5 and R.nt_fast(c) for c in cases)
    lone = [c for c in cases if c["K2"] > 0 and c["offa2"] == 1 and c["offa"] == c["offb"] == c["offb2"] == 0
            and all(c[k] % 4 == 0 for k in ("lda", "ldb", "lda2", "ldb2"))]
    assert lone and not R.nt_fast(lone[0])                                             # only A2 misaligned
    nwg = {math.ceil(c["M"] / 128) * math.ceil(c["N"] / 128) for c in cases if c["K"] == 8}
    assert nwg == {1, 7, 8, 9, 12, 15, 17}
    rem = {(n % 8 != 0, n // 8 != 0) for n in nwg}                                     # (rr != 0, q != 0)
    assert {(False, True), (True, False), (True, True)} <= rem
    assert any(c["bias"] for c in cases) and any(not c["bias"] for c in cases)
