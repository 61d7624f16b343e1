"""GPU: SwitchableLayerNorm under autograd on the HIP forward / backward pair (spq_layernorm_fwd_stats, spq_layernorm_bwd):
train / eval forward identity, launch trace, gradients against the reference's autograd (fixtures) and the oracle's at size,
determinism and batch invariance, partial needs, C-ABI refusals, NaN, autocast, checkpointing and a whole-block step.

The bar everywhere is the project's gradient bar |d| <= 1e-5 |ref| + 1e-5 rms(ref) (tests/ln_grad_ref.py), no element excluded."""
import json
import os
import types

import numpy as np
import pytest
import torch

import ln_grad_ref as R
from test_blocks_cpu import load_blk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    return p


def make_ln(pkg, cols, weight=None, bias=None, levels=(4, 8, 32), seed=5):
    ln = pkg.SwitchableLayerNorm(cols, precision_levels=list(levels), eps=EPS)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in levels:
            ln.weights[str(p)].copy_(torch.randn(cols, generator=gen) * 0.2 + 1.0 if weight is None else weight)
            ln.biases[str(p)].copy_(torch.randn(cols, generator=gen) * 0.1 if bias is None else bias)
    ln = ln.to(DEV)
    ln.set_precision(levels[0])
    return ln


def module_grads(ln, x, g, need=(True, True, True)):
    """(y, dx, dweight, dbias) of one forward + backward of the module at its current precision; None where not needed."""
    key = str(ln.current_precision)
    w, b = ln.weights[key], ln.biases[key]
    saved = (w.requires_grad, b.requires_grad)
    w.requires_grad_(need[1]); b.requires_grad_(need[2])
    w.grad = None; b.grad = None
    xs = x.detach().clone().requires_grad_(need[0])
    y = ln(xs)
    y.backward(g)
    out = (y.detach(), xs.grad, w.grad, b.grad)
    w.grad = None; b.grad = None
    w.requires_grad_(saved[0]); b.requires_grad_(saved[1])
    return out


def cabi_fwd_stats(pkg, x, w, b):
    rows, cols = x.numel() // w.numel(), w.numel()
    out, mean, den = torch.empty_like(x), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    rc = pkg._lib.load().spq_layernorm_fwd_stats(x.data_ptr(), rows, cols, w.data_ptr(), b.data_ptr(), EPS, out.data_ptr(),
                                                 mean.data_ptr(), den.data_ptr(), pkg._lib.stream_ptr(x.device))
    pkg._lib.check(rc, "spq_layernorm_fwd_stats")
    return out, mean, den


# ---- 1. forward identity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [64, 68, 768, 1024, 3072, 8192])
def test_train_forward_is_the_eval_forward(pkg, cols):
    ln = make_ln(pkg, cols)
    lib = pkg._lib.load()
    for rows in [1, 3, 4, 5, 4099] + ([32768] if cols == 768 else []):
        x = (R.make_input("normal", rows, cols, seed=rows + cols) * 1.7 + 0.3).to(DEV)
        x[:, 3] += 25.0
        for p in ln.precision_levels:
            ln.set_precision(p)
            with torch.no_grad():
                y_eval = ln(x)
            y_train = ln(x.clone().requires_grad_(True))
            assert type(y_train.grad_fn).__name__.startswith("_LayerNormFunction"), type(y_train.grad_fn)
            assert torch.equal(y_train.detach(), y_eval), (rows, cols, p)
        # C ABI: out is spq_layernorm's, and mean / den are exactly the numbers the formula needs
        w, b = ln.weights[str(p)].detach(), ln.biases[str(p)].detach()
        out, mean, den = cabi_fwd_stats(pkg, x, w, b)
        out0 = torch.empty_like(x)
        pkg._lib.check(lib.spq_layernorm(x.data_ptr(), rows, cols, w.data_ptr(), b.data_ptr(), EPS, out0.data_ptr(),
                                         pkg._lib.stream_ptr(x.device)), "spq_layernorm")
        assert torch.equal(out, out0) and torch.equal(out, y_eval)
        assert torch.equal(w * ((x - mean[:, None]) / den[:, None]) + b, out), (rows, cols)


# ---- 2. launch trace -----------------------------------------------------------------------------------------------------------
def _launched(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


@pytest.mark.parametrize("cols", [768, 3072])
def test_forward_backward_launch_the_librarys_kernels(pkg, cols):
    ln = make_ln(pkg, cols)
    x, g, _, _ = R.make_case("normal", 256, cols, 3)
    x, g = x.to(DEV), g.to(DEV)
    module_grads(ln, x, g)                                     # warm-up (workspace allocation)
    names = _launched(lambda: module_grads(ln, x, g))
    assert sum("layernorm_stats_kernel" in n for n in names) == 1, names
    assert sum("ln_bwd_rows_kernel" in n for n in names) == 1, names
    assert sum("ln_bwd_merge_kernel" in n for n in names) == 1, names
    assert sum("ln_bwd_cols_kernel" in n for n in names) == (1 if cols > 2048 else 0), names
    for n in names:                                            # no quiet fall-back to the composed formula
        low = n.lower()
        assert not any(k in low for k in ("mean", "var", "welford", "sqrt", "div", "reduce")), n
    ln.fuse_backward = False                                   # the switch restores it
    assert not any("layernorm_stats_kernel" in n or "ln_bwd" in n for n in _launched(lambda: module_grads(ln, x, g)))


# ---- 3. gradients against the reference's fixtures -----------------------------------------------------------------------------
def _check_case(pkg, x, g, w, b, what, judged=None):
    refs, limit, ratio, which = judged if judged is not None else R.yardstick(x, g, w, b, EPS)
    ln = make_ln(pkg, w.numel(), w, b)
    y, dx, dw, db = module_grads(ln, x.to(DEV), g.to(DEV))
    got = [R.bar_ratio(a, r) for a, r in zip((dx, dw, db), refs)]
    print(f"{what}: yardstick {which} (fp32 reference at {ratio:.3f} of the bar against fp64), err/bound dx {got[0]:.3f} "
          f"dweight {got[1]:.3f} dbias {got[2]:.3f}, allowed {limit:.3f}")
    for v, name in zip(got, ("dx", "dweight", "dbias")):
        assert v <= limit, f"{what}: {name} err/bound {v:.3f} > {limit:.3f} against {which}"
    return which


@pytest.mark.parametrize("name", ["768", "1024", "64", "768_channel", "768_offset"])
def test_gradients_against_reference_fixture(pkg, name, golden_dir):
    with np.load(os.path.join(golden_dir, f"lngrad_{name}.npz")) as z:
        meta = json.loads(str(z["meta"]))
        t = {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}
    ratio, which = meta["ref_ratio_vs_fp64"], meta["yardstick"]
    assert (which == "fp32") == (ratio <= R.FP32_REF_LIMIT) and (which == "fp64") == (name == "768_offset")
    if which == "fp32":                                        # the yardstick is the reference's own stored result
        judged = ([t["dx"], t["dweight"], t["dbias"]], 1.0, ratio, which)
    else:                                                      # fp64, widened by the reference's recorded err/bound
        judged = (R.oracle_grads(t["x"], t["g"], t["weight"], t["bias"], EPS, torch.float64)[1:], 1.0 + ratio, ratio, which)
    _check_case(pkg, t["x"], t["g"], t["weight"], t["bias"], f"lngrad_{name}", judged)
    if which == "fp32":   # the forward bound of test_gpu_blocks.py::test_layernorm_kernel; it is a bound for well-conditioned rows
        # (with 0.1 randn + 5 an error of one ulp in the mean is 3e-6 of the row's spread, in the reference as in the kernel)
        ln = make_ln(pkg, meta["C"], t["weight"], t["bias"])
        y = module_grads(ln, t["x"].to(DEV), t["g"].to(DEV))[0]
        d = (y.cpu().double() - t["y"].double()).abs()
        assert bool((d <= 2e-6 * t["y"].double().abs() + 2e-6).all())


# ---- 4. the oracle at size -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", R.DISTRIBUTIONS)
@pytest.mark.parametrize("rows,cols", [(8192, 768), (32768, 768), (8192, 1024), (4096, 3072), (257, 8192), (1000, 68)])
def test_gradients_against_oracle_at_size(pkg, rows, cols, dist):
    x, g, w, b = R.make_case(dist, rows, cols, seed=rows + cols)
    _check_case(pkg, x, g, w, b, f"{rows}x{cols} {dist}")


def test_offset_rows_are_judged_against_fp64(pkg):
    """0.1 randn + 5: x - mean cancels, the fp32 reference itself sits near the bar; not dropped, judged against fp64."""
    x, g, w, b = R.make_case("normal", 2048, 768, seed=77)
    assert _check_case(pkg, x * 0.1 + 5.0, g, w, b, "2048x768 offset") == "fp64"


# ---- 5. determinism and invariance ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [768, 1024, 3072])
def test_deterministic_and_batch_invariant(pkg, cols):
    Rr = 1029
    x, g, w, b = R.make_case("outliers", 4 * Rr, cols, seed=cols)
    ln = make_ln(pkg, cols, w, b)
    x, g = x.to(DEV), g.to(DEV)
    a = module_grads(ln, x, g)
    bb = module_grads(ln, x, g)
    assert all(torch.equal(p, q) for p, q in zip(a, bb)), "two identical calls differ"
    small = module_grads(ln, x[:Rr], g[:Rr])
    assert torch.equal(small[1], a[1][:Rr]), "dx of a row depends on the other rows of the call"
    # column sums: a 2R-row call against the sum of its two halves.  Not expected bit-equal (the slab cut of 2R rows is not the
    # union of the cuts of the halves): equal at the bar.
    both = module_grads(ln, x[:2 * Rr], g[:2 * Rr])
    second = module_grads(ln, x[Rr:2 * Rr], g[Rr:2 * Rr])
    for i, name in ((2, "dweight"), (3, "dbias")):
        v = R.bar_ratio(small[i] + second[i], both[i])
        assert v <= 1.0, (name, v)


# ---- 6. partial needs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [768, 3072])
def test_partial_needs(pkg, cols):
    x, g, w, b = R.make_case("normal", 515, cols, seed=9)
    ln = make_ln(pkg, cols, w, b)
    x, g = x.to(DEV), g.to(DEV)
    full = module_grads(ln, x, g)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        got = module_grads(ln, x, g, need)
        assert torch.equal(got[0], full[0])
        for i in range(3):
            if need[i]:
                assert got[i + 1].is_contiguous() and got[i + 1].dtype == torch.float32
                assert torch.equal(got[i + 1], full[i + 1]), (need, i)
            else:
                assert got[i + 1] is None, (need, i)


# ---- 7. C-ABI refusals ---------------------------------------------------------------------------------------------------------
def test_cabi_refusals_touch_nothing(pkg):
    lib = pkg._lib.load()
    rows, cols, SENT = 64, 768, -777.0
    x, g, w, b = (t.to(DEV) for t in R.make_case("normal", rows, cols, seed=1))
    _, mean, den = cabi_fwd_stats(pkg, x, w, b)
    need = lib.spq_layernorm_bwd_workspace_bytes(rows, cols)
    ws = torch.empty(need + 64, dtype=torch.uint8, device=DEV)
    g_off = torch.empty(rows * cols + 4, device=DEV)[1:]        # 4 bytes past a 16-byte boundary
    assert g_off.data_ptr() % 16 == 4
    outs = [torch.full((rows, cols), SENT, device=DEV), torch.full((cols,), SENT, device=DEV), torch.full((cols,), SENT, device=DEV)]
    st = pkg._lib.stream_ptr(torch.device(DEV))
    P = lambda t: t.data_ptr()

    def bwd(g_=g, x_=x, cols_=cols, nbytes=need, dx=outs[0]):
        return lib.spq_layernorm_bwd(None if g_ is None else P(g_), None if x_ is None else P(x_), P(mean), P(den), P(w), rows, cols_,
                                     P(dx), P(outs[1]), P(outs[2]), P(ws), nbytes, st)
    cases = [("null g", lambda: bwd(g_=None), -1, b"null pointer"), ("null x", lambda: bwd(x_=None), -1, b"null pointer"),
             ("cols = 6", lambda: bwd(cols_=6), -3, b"cols"), ("cols = 8196", lambda: bwd(cols_=8196), -3, b"cols"),
             ("misaligned g", lambda: bwd(g_=g_off), -3, b"aligned"), ("short workspace", lambda: bwd(nbytes=need - 1), -5, b"workspace")]
    for what, call, code, word in cases:
        rc = call()
        assert rc == code, (what, rc, lib.spq_last_error())
        assert word in lib.spq_last_error(), (what, lib.spq_last_error())
    out, m2, d2 = torch.full((rows, cols), SENT, device=DEV), torch.full((rows,), SENT, device=DEV), torch.full((rows,), SENT, device=DEV)
    for cols_ in (6, 8196):
        assert lib.spq_layernorm_fwd_stats(P(x), rows, cols_, P(w), P(b), EPS, P(out), P(m2), P(d2), st) == -3
    assert lib.spq_layernorm_fwd_stats(P(x), rows, cols, P(w), P(b), EPS, P(out), None, P(d2), st) == -1
    torch.cuda.synchronize()
    for t in outs + [out, m2, d2]:
        assert bool((t == SENT).all()), "a refused call wrote to an output"
    assert bwd() == 0                                           # and the same call, valid, runs
    torch.cuda.synchronize()
    assert not bool((outs[0] == SENT).any())


# ---- 8. NaN --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [768, 3072])
def test_nan_follows_torch(pkg, cols):
    """A NaN in one row of x: that dx row is NaN, every other dx row is bit-identical to the clean call, dweight is NaN in every
    column (x_hat of the whole row is NaN).  dbias = sum of g does not involve x: torch leaves it finite and so do the kernels --
    checked against the composed formula's NaN pattern on the same device.  A NaN in g: dx row NaN, that column of dweight AND
    dbias NaN, all other columns finite."""
    x, g, w, b = R.make_case("normal", 300, cols, seed=4)
    ln = make_ln(pkg, cols, w, b)
    x, g = x.to(DEV), g.to(DEV)
    clean = module_grads(ln, x, g)
    xn = x.clone(); xn[17, 5] = float("nan")
    got = module_grads(ln, xn, g)
    keep = torch.ones(300, dtype=torch.bool, device=DEV); keep[17] = False
    assert bool(torch.isnan(got[1][17]).all()) and torch.equal(got[1][keep], clean[1][keep])
    assert bool(torch.isnan(got[2]).all())
    ln.fuse_backward = False
    composed = module_grads(ln, xn, g)
    ln.fuse_backward = True
    for i in (1, 2, 3):
        assert torch.equal(torch.isnan(got[i]), torch.isnan(composed[i])), i
    assert torch.equal(got[3], clean[3])
    gn = g.clone(); gn[33, 9] = float("nan")
    got = module_grads(ln, x, gn)
    keep[17] = True; keep[33] = False
    assert bool(torch.isnan(got[1][33]).all()) and torch.equal(got[1][keep], clean[1][keep])
    col = torch.zeros(cols, dtype=torch.bool, device=DEV); col[9] = True
    assert torch.equal(torch.isnan(got[2]), col) and torch.equal(torch.isnan(got[3]), col)


# ---- 9. autocast, half input, checkpointing, double backward -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_autocast_keeps_fp32(pkg, dtype):
    x, g, w, b = R.make_case("normal", 130, 768, seed=2)
    ln = make_ln(pkg, 768, w, b)
    x, g = x.to(DEV), g.to(DEV)
    plain = module_grads(ln, x, g)
    with torch.autocast("cuda", dtype=dtype):
        xs = x.clone().requires_grad_(True)
        y = ln(xs)
        assert y.dtype == torch.float32 and type(y.grad_fn).__name__.startswith("_LayerNormFunction")
    y.backward(g)
    key = str(ln.current_precision)
    got = (y.detach(), xs.grad, ln.weights[key].grad, ln.biases[key].grad)
    for p, q in zip(got, plain):
        assert p.dtype == torch.float32 and torch.equal(p, q)
    ln.zero_grad(set_to_none=True)
    yh = ln(x.to(dtype).requires_grad_(True))                  # a half input: the composed formula, as before
    assert yh.grad_fn is not None and not type(yh.grad_fn).__name__.startswith("_LayerNormFunction")


def test_double_backward_raises(pkg):
    ln = make_ln(pkg, 64)
    xs = torch.randn(8, 64, device=DEV, requires_grad=True)
    (gx,) = torch.autograd.grad(ln(xs).sum(), xs, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def _train_block(pkg, name="block_mm4"):
    meta, t = load_blk(name)
    bits, r = meta["bits"], meta["r"]
    cfg = types.SimpleNamespace(n_embd=meta["E"], n_head=meta["H"], n_positions=meta["n_positions"], layer_norm_epsilon=1e-5,
                                bit_widths=[bits, 32], lora_rank_per_bit={bits: r, 32: 0}, lora_alpha_per_bit={bits: meta["alpha"], 32: 0},
                                quantizer_per_bit={bits: meta["qtype"], 32: None}, per_channel_quantization=True)
    blk = pkg.SPBlock(cfg, bit_widths=[bits, 32])
    with torch.no_grad():
        for n, p_ in blk.named_parameters():
            p_.copy_(t[f"param.{n}"])
    blk = blk.to(DEV).eval()
    pkg.calibrate_model(blk, bits, [t["x0"].to(DEV), t["x1"].to(DEV)])   # as test_gpu_blocks.py does
    blk.train()
    for lin in (blk.attn.c_attn, blk.attn.c_proj, blk.mlp.c_fc, blk.mlp.c_proj):     # base weights frozen (main_sp.py:83)
        lin.linear.weight.requires_grad_(False)
        if lin.linear.bias is not None:
            lin.linear.bias.requires_grad_(False)
    return blk, t, bits


def _block_step(blk, x, g, use_checkpoint=False, capture=None):
    blk.zero_grad(set_to_none=True)
    xs = x.detach().clone().requires_grad_(True)
    hooks = []
    if capture is not None:
        for nm, mod, post in (("c_attn", blk.ln_1, True), ("attn.c_proj", blk.attn.c_proj, False), ("c_fc", blk.ln_2, True),
                              ("mlp.c_proj", blk.mlp.c_proj, False)):
            if post:
                hooks.append(mod.register_forward_hook(lambda m, a, out, nm=nm: capture.__setitem__(nm, out.detach())))
            else:
                hooks.append(mod.register_forward_pre_hook(lambda m, a, nm=nm: capture.__setitem__(nm, a[0].detach())))
    y = blk(xs, None, use_checkpoint)
    for h in hooks:
        h.remove()
    y.backward(g)
    grads = {n: p.grad.clone() for n, p in blk.named_parameters() if p.grad is not None}
    grads["input"] = xs.grad.clone()
    return y.detach(), grads


def test_checkpointing_gives_the_same_gradients(pkg):
    blk, t, bits = _train_block(pkg)
    x = t["x2"].to(DEV)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(8)).to(DEV)
    y0, g0 = _block_step(blk, x, g, use_checkpoint=False)
    y1, g1 = _block_step(blk, x, g, use_checkpoint=True)
    assert torch.equal(y0, y1) and sorted(g0) == sorted(g1)
    assert any("ln_1.weights" in n for n in g0) and any("lora_A" in n for n in g0)
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ---- 10. a whole block's training step, HIP pair against the composed formula --------------------------------------------------
def test_block_step_against_composed_layernorm(pkg):
    """The two runs are NOT expected bit-identical: the composed forward is ulps from the kernel's, which can flip an input level of
    a linear and move that row by a quantisation step.  Rows whose input levels of the four linears are identical in both runs are
    compared at the bar; the others are left out (their incoming gradient zeroed in both runs, since parameter gradients sum over
    rows), their share printed and capped at 5 %."""
    blk, t, bits = _train_block(pkg)
    key = f"{bits}bit"
    x = t["x2"].to(DEV)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(21)).to(DEV)
    lins = {"c_attn": blk.attn.c_attn, "attn.c_proj": blk.attn.c_proj, "c_fc": blk.mlp.c_fc, "mlp.c_proj": blk.mlp.c_proj}

    def run(fuse, gg):
        blk.ln_1.fuse_backward = blk.ln_2.fuse_backward = fuse
        cap = {}
        y, grads = _block_step(blk, x, gg, capture=cap)
        with torch.no_grad():
            lv = {n: lins[n].quantizers_input[key].quantize_levels(cap[n].contiguous()).reshape(cap[n].shape) for n in lins}
        return y, grads, lv
    _, _, lv_a = run(True, g)
    _, _, lv_b = run(False, g)
    left_out = torch.zeros(x.shape[:-1], dtype=torch.bool, device=DEV)
    for n in lins:
        left_out |= (lv_a[n] != lv_b[n]).any(dim=-1).reshape(left_out.shape)
    share = float(left_out.float().mean())
    print(f"block step: {int(left_out.sum())} of {left_out.numel()} rows left out ({100 * share:.2f} %)")
    assert share <= 0.05
    gm = g * (~left_out).unsqueeze(-1)
    _, ga, _ = run(True, gm)
    _, gb, _ = run(False, gm)
    assert sorted(ga) == sorted(gb)
    checked = 0
    for n in ga:
        if n == "input" or ".weights." in n or ".biases." in n or "lora_" in n:
            a, b_ = ga[n], gb[n]
            if n == "input":
                a, b_ = a[~left_out], b_[~left_out]
            v = R.bar_ratio(a, b_)
            print(f"  {n}: err/bound {v:.3f}")
            assert v <= 1.0, (n, v)
            checked += 1
    assert checked >= 1 + 4 + 8
