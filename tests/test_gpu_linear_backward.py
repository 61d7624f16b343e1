"""GPU: the backward of SPLinearWithLoRA (sp_linear.py) and CPTLinear (cpt.py), the limb GEMM it rests on, and the LoRA-down product the
forward saves for it, against the float64 closed form of tests/linear_grad_ref.py fed the product's OWN fake-quantised operands.

The bar is the project's: |d| <= 1e-5 |ref| + 1e-5 rms(ref) (helpers.assert_close_y).  Where a gradient is clamped to +-10 -- the
straight-through estimator of a log quantiser -- and the inputs are scaled so that the clamp is ACTIVE on a quarter to a third of the
elements (linear_grad_ref.sp_clamp_inputs / cpt_clamp_inputs), the bound is taken at the scale of the clamp's argument:
|d| <= 1e-5 |pre| + 1e-5 rms(pre).  Clamping is 1-Lipschitz, so that bound carries over from the argument to the result; a bound at the
scale of the saturated result is one no fp32 implementation meets.  For SPLinearWithLoRA's d/dx, clamp(g . FQ(W)) + adapter term, ``pre``
is |g . FQ(W)| + |adapter term|.  A backward without the clamp, one that clamps after adding the adapter term, and a CPTLinear backward
that clamps nothing all fail here.

Every test prints its worst err/bound per output."""
import pytest
import torch

import linear_grad_ref as R
from helpers import assert_close_y

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    yield p
    print("\nworst err/bound per output over this file: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


def close(got, ref, what, out, pre=None):
    """the bar; ``pre``: the argument of the clamp that produced ``ref`` (active-clamp inputs), else the reference itself"""
    assert got is not None, f"{what}: no gradient"
    got = got.reshape(ref.shape)
    if pre is None:
        w = assert_close_y(got, ref, what, 1e-5)
    else:
        w = R.worst_ratio(got, ref, pre)
        assert w <= 1.0, f"{what}: max err/bound = {w:.3f} at the pre-clamp scale"
    WORST[out] = max(WORST.get(out, 0.0), w)
    return w


# ---------------------------------------------------------------------------------------------------------------------
# _LimbGemm
# ---------------------------------------------------------------------------------------------------------------------
def _rows_within_16(M, C, gen):
    """randn rows, each normalised to max |.| = 1 and then scaled by a factor in [1, 16]: the accuracy of rows far below the batch
    maximum is a separate, known matter (test_gpu_batch_invariance.py)"""
    a = torch.randn(M, C, generator=gen)
    a = a / a.abs().amax(dim=1, keepdim=True).clamp(min=1e-3)
    f = torch.exp2(4.0 * torch.rand(M, 1, generator=gen))
    f[0] = 16.0
    a = a * f
    mx = a.abs().amax(dim=1)
    assert float(mx.max() / mx.min()) <= 16.0 + 1e-4
    return a


@pytest.mark.parametrize("with_down", [False, True], ids=["plain", "down"])
@pytest.mark.parametrize("M,C,R_,r", R.LIMB_SHAPES, ids=lambda v: str(v))
def test_limb_gemm_against_float64(pkg, M, C, R_, r, with_down):
    from llm_qat_on_gpt2_amd.sp_linear import _LimbGemm
    assert _LimbGemm.supported(R_, C)
    gen = torch.Generator().manual_seed(M + C + R_ + r)
    a = _rows_within_16(M, C, gen).to(DEV)
    b = (torch.randn(R_, C, generator=gen) * 0.05).to(DEV)
    down = (torch.randn(r, C, generator=gen) * 0.05).to(DEV)
    gm = _LimbGemm()
    res = gm(a, b, down=down) if with_down else gm(a, b)
    out, t = res if with_down else (res, None)
    torch.cuda.synchronize()
    w = close(out, a.double() @ b.double().t(), f"limb({M},{C},{R_})", "limb_out")
    msg = f"limb gemm ({M},{C},{R_},{r}) down={with_down}: out err/bound {w:.3f}"
    if with_down:
        msg += f", t err/bound {close(t, a.double() @ down.double().t(), f'limb_t({M},{C},{r})', 'limb_t'):.3f}"
        again, t2 = gm(a, b, down=down)
        assert torch.equal(again, out) and torch.equal(t2, t)
    print(msg)


def test_limb_gemm_on_integers_report_only(pkg):
    """integer operands, where fp32 itself is exact: prints whether the two-limb product is, and asserts the bar only"""
    from llm_qat_on_gpt2_amd.sp_linear import _LimbGemm
    gen = torch.Generator().manual_seed(1)
    a = torch.randint(-3, 4, (129, 132), generator=gen).float().to(DEV)
    b = torch.randint(-3, 4, (96, 132), generator=gen).float().to(DEV)
    down = torch.randint(-3, 4, (16, 132), generator=gen).float().to(DEV)
    out, t = _LimbGemm()(a, b, down=down)
    ro, rt = a.double() @ b.double().t(), a.double() @ down.double().t()
    print(f"limb gemm on integers: out bit-exact {bool(torch.equal(out.double(), ro))}, t bit-exact {bool(torch.equal(t.double(), rt))}")
    close(out, ro, "limb(int)", "limb_out")
    close(t, rt, "limb_t(int)", "limb_t")


# ---------------------------------------------------------------------------------------------------------------------
# SPLinearWithLoRA
# ---------------------------------------------------------------------------------------------------------------------
SP_QUANT = [("mm4_pc", 4, "minmax", True), ("mm4_pt", 4, "minmax", False), ("mm8_pc", 8, "minmax", True), ("mm8_pt", 8, "minmax", False),
            ("log6_pc", 6, "log", True), ("log6_pt", 6, "log", False)]


def build_sp(pkg, shape, bits, qtype, per_channel, seed=3, path=None):
    M, K, N, r = shape
    W, bias, A, B, x, x_cal, g = R.make_inputs(M, K, N, r, seed)
    layer = pkg.SPLinearWithLoRA(K, N, [bits, 32], {bits: r, 32: 0}, {bits: 2 * r, 32: 0}, {bits: qtype, 32: None}, per_channel=per_channel)
    key = f"{bits}bit"
    with torch.no_grad():
        layer.linear.weight.copy_(W); layer.linear.bias.copy_(bias)
        layer.lora_adapters[key].lora_A.copy_(A); layer.lora_adapters[key].lora_B.copy_(B)
    layer = layer.to(DEV).train()
    layer.set_precision(bits)
    if path is not None:
        layer.operand_path = path
    pkg.calibrate_layer(layer, bits, [x.to(DEV), x_cal.to(DEV)])
    return layer, key, x.to(DEV), g.to(DEV)


def sp_reference(layer, key, x, g, use_lora=True):
    """the closed form on the product's own FQ tensors"""
    qx, qw, lo = layer.quantizers_input[key], layer.quantizers_weight[key], layer.lora_adapters[key]
    K, N = layer.in_features, layer.out_features
    is_log = qx.quantizer_type == "log"
    with torch.no_grad():
        x2 = x.reshape(-1, K)
        wq, xq = qw(layer.linear.weight), qx(x2).reshape(-1, K)
        aq = lo.quantize_A(lo.lora_A) if use_lora else None
        bq = lo.quantize_B(lo.lora_B) if use_lora else None
    return R.sp_backward(g.reshape(-1, N), wq, x2, xq, aq, bq, float(lo.scaling) if use_lora else 0.0, is_log, is_log, is_log, is_log)


def g_as(form, g, y_shape):
    """the incoming gradient as autograd may hand it over; ``None``: y.sum().backward(), an expanded stride-0 tensor of ones"""
    g = g.reshape(y_shape)
    if form == "dense":
        return g.contiguous()
    if form == "sliced":
        big = torch.zeros(*y_shape[:-1], y_shape[-1] + 3, device=g.device)
        big[..., :y_shape[-1]] = g
        v = big[..., :y_shape[-1]]
        assert not v.is_contiguous() or v.shape[:-1].numel() == 1
        return v
    assert form == "ones"
    return None


def sp_run(layer, key, x, g, need=("x", "A", "B"), form="dense", three_d=False):
    """one forward + backward; returns (grads by name, the g that was applied as [M, N])"""
    lo = layer.lora_adapters[key]
    M, K = x.shape
    for name, p in (("W", layer.linear.weight), ("b", layer.linear.bias), ("A", lo.lora_A), ("B", lo.lora_B)):
        p.requires_grad_(name in need)
        p.grad = None
    xin = x.clone()
    if three_d:
        xin = xin.view((2, M // 2, K) if M % 2 == 0 else (1, M, K))
    xin.requires_grad_("x" in need)
    y = layer(xin)
    assert "SPLinearFunction" in type(y.grad_fn).__name__
    gv = g_as(form, g, y.shape)
    if gv is None:
        y.sum().backward()
        g = torch.ones_like(g)
    else:
        y.backward(gv)
    grads = {"x": xin.grad, "W": layer.linear.weight.grad, "b": layer.linear.bias.grad, "A": lo.lora_A.grad, "B": lo.lora_B.grad}
    for name in grads:
        assert (grads[name] is not None) == (name in need), f"gradient of {name}: needed {name in need}"
    return grads, g


def sp_check(grads, ref, what, clamped=False):
    """compare whatever gradients are there; ``clamped``: bounds at the pre-clamp scale"""
    pre = (lambda n: ref[n]) if clamped else (lambda n: None)
    ws = {}
    if grads["x"] is not None:
        ws["gx"] = close(grads["x"], ref["gx"], what + ".gx", "sp_gx", pre("pre_gx"))
    if grads["A"] is not None:
        ws["gA"] = close(grads["A"], ref["gA"], what + ".gA", "sp_gA", pre("pre_gA"))
    if grads["B"] is not None:
        ws["gB"] = close(grads["B"], ref["gB"], what + ".gB", "sp_gB", pre("pre_gB"))
    if grads["W"] is not None:
        ws["gW"] = close(grads["W"], ref["gW"], what + ".gW", "sp_gW", pre("pre_gW"))
    if grads["b"] is not None:
        ws["gb"] = close(grads["b"], ref["gb"], what + ".gb", "sp_gb")
    return ws


def sp_all_modes(layer, key, x, g, what, clamped=False):
    """every gradient requirement, every form of the incoming gradient, 2-D and 3-D x, both d/dx kernels, and determinism"""
    ones = torch.ones_like(g)
    ref = sp_reference(layer, key, x, g)
    report = {}

    def upd(ws):
        for k, v in ws.items():
            report[k] = max(report.get(k, 0.0), v)
    grads, _ = sp_run(layer, key, x, g, ("x", "A", "B"), "dense", three_d=True)
    upd(sp_check(grads, ref, what + "[xAB]", clamped))
    again, _ = sp_run(layer, key, x, g, ("x", "A", "B"), "dense", three_d=True)
    for n in ("x", "A", "B"):
        assert torch.equal(grads[n], again[n]), f"{what}: two backward runs differ in d/d{n}"
    grads, _ = sp_run(layer, key, x, g, ("A", "B"), "sliced", three_d=True)           # gt from the fp32 kernel, no d/dx at all
    upd(sp_check(grads, ref, what + "[AB,sliced g]", clamped))
    grads, _ = sp_run(layer, key, x, g, ("x", "W", "b", "A", "B"), "sliced")
    upd(sp_check(grads, ref, what + "[xWbAB]", clamped))
    layer.backward_limbs = False
    grads, _ = sp_run(layer, key, x, g, ("x", "A", "B"), "dense")
    upd(sp_check(grads, ref, what + "[xAB,fp32 d/dx]", clamped))
    layer.backward_limbs = True
    if not clamped:                                                                   # a gradient of ones has no scale to set
        grads, _ = sp_run(layer, key, x, ones, ("x",), "ones")
        upd(sp_check(grads, sp_reference(layer, key, x, ones), what + "[x,sum()]"))
    else:
        grads, _ = sp_run(layer, key, x, g, ("x",), "dense")
        upd(sp_check(grads, ref, what + "[x]", clamped))
    layer.calibration_mode = True                                                     # the adapter off: use_lora false
    try:
        for limbs in (True, False):
            layer.backward_limbs = limbs
            grads, _ = sp_run(layer, key, x, g, ("x", "W"), "dense", three_d=limbs)
            upd(sp_check(grads, sp_reference(layer, key, x, g, use_lora=False), what + f"[no adapter, limbs={limbs}]", clamped))
    finally:
        layer.calibration_mode = False
        layer.backward_limbs = True
    print(f"{what}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in report.items()))
    return ref


@pytest.mark.parametrize("qname,bits,qtype,per_channel", SP_QUANT, ids=[q[0] for q in SP_QUANT])
@pytest.mark.parametrize("shape", R.SP_SHAPES, ids=lambda v: str(v))
def test_sp_backward_against_float64(pkg, shape, qname, bits, qtype, per_channel):
    layer, key, x, g = build_sp(pkg, shape, bits, qtype, per_channel)
    assert float(layer.lora_adapters[key].lora_B.detach().abs().max()) > 0             # random B, not the zero initialisation
    sp_all_modes(layer, key, x, g, f"sp {shape} {qname}")


@pytest.mark.parametrize("per_channel", [True, False], ids=["pc", "pt"])
@pytest.mark.parametrize("shape", R.SP_CLAMP_SHAPES, ids=lambda v: str(v))
def test_sp_backward_with_every_clamp_active(pkg, shape, per_channel):
    layer, key, x, g = build_sp(pkg, shape, 6, "log", per_channel)
    lo, qw = layer.lora_adapters[key], layer.quantizers_weight[key]
    s = float(lo.scaling)

    def fq_b(B):
        with torch.no_grad():
            lo.lora_B.copy_(B.to(DEV))
            q = lo.quantize_B
            q.start_calibration(); q(lo.lora_B); q.finish_calibration()
            return q(lo.lora_B).cpu()
    with torch.no_grad():
        wq, aq = qw(layer.linear.weight).cpu(), lo.quantize_A(lo.lora_A).cpu()
    g, x, B = R.sp_clamp_inputs(g.cpu(), x.cpu(), lo.lora_B.detach().cpu(), wq, aq, s, fq_b)
    with torch.no_grad():
        lo.lora_B.copy_(B.to(DEV))
    x, g = x.to(DEV), g.to(DEV)
    pkg.calibrate_layer(layer, 6, [x])                                                # every quantiser on what it will see
    ref = sp_reference(layer, key, x, g)
    shares = {n: R.share_outside(ref[n]) for n in ("pre_base", "pre_gA", "pre_gB")}
    for n, sh in shares.items():
        assert 0.10 <= sh <= 0.60, f"sp {shape}: {sh:.3f} of {n} lies outside +-10"
    with torch.no_grad():
        wrong = R.sp_backward_wrong_order(g, qw(layer.linear.weight), lo.quantize_A(lo.lora_A), lo.quantize_B(lo.lora_B), s)
    bound = 1e-5 * ref["pre_gx"] + 1e-5 * float(ref["pre_gx"].pow(2).mean().sqrt())
    far = float(((wrong - ref["gx"]).abs() > bound).double().mean())
    assert far >= 0.20, f"sp {shape}: clamp(base + lora) differs from clamp(base) + lora on only {far:.3f} of d/dx"
    print(f"sp {shape} active clamp: shares " + ", ".join(f"{n} {v:.3f}" for n, v in shares.items()) + f"; wrong-order share {far:.3f}")
    sp_all_modes(layer, key, x, g, f"sp {shape} log6_{'pc' if per_channel else 'pt'} active clamp", clamped=True)


# ---------------------------------------------------------------------------------------------------------------------
# The LoRA-down product the training forward saves for d/dB, on every operand path
# ---------------------------------------------------------------------------------------------------------------------
def _t_paths(L):
    return [("f32", L.PATH_F32, 8, "minmax", True), ("f16x2", L.PATH_F16X2, 8, "minmax", True), ("f16x3", L.PATH_F16X3, 6, "log", True),
            ("i8", L.PATH_I8, 8, "minmax", False), ("fp6", L.PATH_FP6, 4, "minmax", True)]


@pytest.mark.parametrize("K", [96, 100])
@pytest.mark.parametrize("r", [1, 16, 63, 128])
@pytest.mark.parametrize("pname", ["f32", "f16x2", "f16x3", "i8", "fp6"])
def test_saved_lora_down_product(pkg, pname, r, K):
    L = pkg._lib
    _, path, bits, qtype, pc = next(p for p in _t_paths(L) if p[0] == pname)
    layer, key, _, _ = build_sp(pkg, (300, K, 72, r), bits, qtype, pc, seed=r + K, path=path)
    qx, qw, lo = layer.quantizers_input[key], layer.quantizers_weight[key], layer.lora_adapters[key]
    assert layer._choose_path(qx, qw, lo, True, 1) == path, f"_choose_path does not allow {pname} here"
    gen = torch.Generator().manual_seed(K + r)
    with torch.no_grad():
        aq = lo.quantize_A(lo.lora_A).double()
        for M in (1, 17, 129, 300):
            x = torch.randn(M, K, generator=gen).to(DEV)
            layer._forward_fused(x, key, qx, qw, lo, keep_t=True)
            t = layer._last_t
            assert layer._last_path == path and t is not None and tuple(t.shape) == (M, r)
            w = close(t, x.double() @ aq, f"t[{pname}, M={M}, r={r}, K={K}]", "t")
            print(f"saved t {pname} M={M} r={r} K={K}: err/bound {w:.3f}")


# ---------------------------------------------------------------------------------------------------------------------
# CPTLinear
# ---------------------------------------------------------------------------------------------------------------------
def build_cpt(pkg, shape, bits, qtype, seed=3):
    M, K, N, r = shape
    W, bias, A, B, x, x_cal, g = R.make_inputs(M, K, N, r, seed, b_nr=True)
    m = pkg.CPTLinear(K, N, bit_widths=[bits, 32], quantizer_per_bit={bits: qtype, 32: None}, shared_lora_rank=r, shared_lora_alpha=2 * r)
    with torch.no_grad():
        m.linear.weight.copy_(W); m.linear.bias.copy_(bias)
        m.shared_lora.lora_A.copy_(A); m.shared_lora.lora_B.copy_(B)
    m = m.to(DEV).train()
    pkg.calibrate_cpt_layer(m, bits, [x.to(DEV), x_cal.to(DEV)])
    m.set_precision(bits)
    return m, x.to(DEV), g.to(DEV)


def cpt_reference(m, x, g):
    lo, ql = m.shared_lora, m.lora_weight_quantizers[f"{m.current_bits}bit"]
    is_log = m.quantizer_input.quantizer_type == "log"
    assert m.quantizer_input.active() and m.quantizer_weight.active() and ql.active()
    assert not lo.grad_quantizer_A.active() and not lo.grad_quantizer_B.active()       # gradient quantisers off
    with torch.no_grad():
        wq, xq = m.quantizer_weight(m.linear.weight), m.quantizer_input(x).reshape(-1, m.in_features)
        aq, bq = ql(lo.lora_A), ql(lo.lora_B)
    return R.cpt_backward(g, wq, xq, aq, bq, float(lo.scaling), is_log, is_log, ql.quantizer_type == "log")


def cpt_run(m, x, g, need):
    lo = m.shared_lora
    for name, p in (("W", m.linear.weight), ("b", m.linear.bias), ("A", lo.lora_A), ("B", lo.lora_B)):
        p.requires_grad_(name in need)
        p.grad = None
    xin = x.clone().requires_grad_("x" in need)
    y = m(xin)
    assert "CPTLinearFunction" in type(y.grad_fn).__name__
    y.backward(g)
    return {"x": xin.grad, "A": lo.lora_A.grad, "B": lo.lora_B.grad, "W": m.linear.weight.grad, "b": m.linear.bias.grad}


def cpt_all_modes(m, x, g, what, clamped=False):
    ref = cpt_reference(m, x, g)
    pre = (lambda n: ref[n]) if clamped else (lambda n: None)
    grads = cpt_run(m, x, g, ("x", "A", "B"))
    ws = {"gx": close(grads["x"], ref["gx"], what + ".gx", "cpt_gx", pre("pre_gx")),
          "gA": close(grads["A"], ref["gA"], what + ".gA", "cpt_gA", pre("pre_gA")),
          "gB": close(grads["B"], ref["gB"], what + ".gB", "cpt_gB", pre("pre_gB"))}
    assert grads["W"] is None and grads["b"] is None
    again = cpt_run(m, x, g, ("x", "A", "B"))
    for n in ("x", "A", "B"):
        assert torch.equal(grads[n], again[n]), f"{what}: two backward runs differ in d/d{n}"
    only = cpt_run(m, x, g, ("x",))
    assert only["A"] is None and only["B"] is None
    ws["gx"] = max(ws["gx"], close(only["x"], ref["gx"], what + ".gx[x only]", "cpt_gx", pre("pre_gx")))
    print(f"{what}: worst err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in ws.items()))


@pytest.mark.parametrize("bits,qtype", [(8, "minmax"), (6, "log")], ids=["mm8", "log6"])
@pytest.mark.parametrize("shape", R.CPT_SHAPES, ids=lambda v: str(v))
def test_cpt_backward_against_float64(pkg, shape, bits, qtype):
    m, x, g = build_cpt(pkg, shape, bits, qtype)
    cpt_all_modes(m, x, g, f"cpt {shape} {qtype}{bits}")


@pytest.mark.parametrize("shape", R.CPT_SHAPES, ids=lambda v: str(v))
def test_cpt_backward_with_every_clamp_active(pkg, shape):
    m, x, g = build_cpt(pkg, shape, 6, "log")
    lo, ql, qi = m.shared_lora, m.lora_weight_quantizers["6bit"], m.quantizer_input

    def fq_l(B):
        with torch.no_grad():
            lo.lora_B.copy_(B.to(DEV))
            ql.start_calibration(); ql(lo.lora_A); ql(lo.lora_B); ql.finish_calibration()
            return ql(lo.lora_A).cpu(), ql(lo.lora_B).cpu()

    def fq_x(xc):
        with torch.no_grad():
            xd = xc.to(DEV)
            qi.start_calibration(); qi(xd); qi.finish_calibration()
            return qi(xd).cpu()
    with torch.no_grad():
        wq = m.quantizer_weight(m.linear.weight).cpu()
    g, x, B = R.cpt_clamp_inputs(g.cpu(), x.cpu(), lo.lora_B.detach().cpu(), wq, float(lo.scaling), fq_l, fq_x)
    with torch.no_grad():
        lo.lora_B.copy_(B.to(DEV))
    x, g = x.to(DEV), g.to(DEV)
    pkg.calibrate_cpt_layer(m, 6, [x])
    m.set_precision(6)
    ref = cpt_reference(m, x, g)
    shares = {n: R.share_outside(ref[n]) for n in ("pre_gx", "pre_gA", "pre_gB")}
    for n, sh in shares.items():
        assert 0.10 <= sh <= 0.60, f"cpt {shape}: {sh:.3f} of {n} lies outside +-10"
    print(f"cpt {shape} active clamp: shares " + ", ".join(f"{n} {v:.3f}" for n, v in shares.items()))
    cpt_all_modes(m, x, g, f"cpt {shape} log6 active clamp", clamped=True)
