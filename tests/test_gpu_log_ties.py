"""Log levels at the rounding ties, against the correctly rounded chain (tests/log_exact.py), bit for bit.

log_level (spq_common.h) decides a level on a fast path (v_log_f32, v_rcp_f32) and sends an element through the fp64 log2 only
when an error bound says the pre-round value may be near a tie.  Every other log test compares with the ATen-based oracle and so
forgives a |delta| = 1 next to a tie -- exactly what a wrong bound produces.  Here the inputs are constructed on and around the
ties (log_exact.tie_matrix: |x| ~ 1, the 1e-5 clamp, |lg| up to ~120, the clamp edges of ln, ranges down to 1e-5) and the levels
must be those of the correctly rounded chain at every site that decides one, outside log_exact's ambiguity mask (reported).
Dequantised values must be within 1 ulp of the correctly rounded exp2 (v_exp_f32's documented accuracy).  Each case also asserts
its coverage: enough elements exactly on k + 1/2, and enough within the device's own bound of one, so that both the fast path
and the fallback run."""
import numpy as np
import pytest
import torch

import log_exact as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIN_EXACT, MIN_NEAR = 100, 1000


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    return p


def _check_coverage(x, mins, ranges, bits, sym, mask=None, what=""):
    x = x if mask is None else np.where(mask, x, np.float32(np.nan))
    exact, near = L.coverage(x, mins, ranges, bits, sym)
    print(f"{what}: {exact} elements on k+1/2, {near} within the device bound")
    assert exact >= MIN_EXACT and near >= MIN_NEAR, (what, exact, near)
    return exact, near


def _expect(x, mins, ranges, bits, sym, direct):
    q = L.levels(x, mins, ranges, bits, sym)
    amb = L.ambiguous(x, mins, ranges, bits, sym)
    return q, L.dequant(x, q, mins, ranges, bits, sym, direct), amb


def _assert_levels(q_dev, q_ref, amb, what):
    bad = (q_dev != q_ref) & ~amb
    if bad.any():
        i = np.argwhere(bad)[:8]
        raise AssertionError(f"{what}: {int(bad.sum())} levels differ from the correctly rounded chain "
                             f"(first at {i.tolist()}: device {q_dev[bad][:8].tolist()} exact {q_ref[bad][:8].tolist()})")


def _assert_dequant(o_dev, o_ref, amb, what):
    d = L.ulp_distance(o_dev, o_ref)
    d = np.where(amb, 0, d)
    assert int(d.max()) <= 1, f"{what}: dequantised value {int(d.max())} ulp from the correctly rounded exp2"


# ---- fakequant_kernel: MODE 0 (ragged generic), 1 (inner == 1, chan % 4 == 0), 2 (inner % 4 == 0 / per-tensor) -------------------
def _fakequant(pkg, x, outer, chan, inner, scale, zp, per_channel, bits, qtype, sym, lb):
    lib = pkg._lib
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    st = torch.from_numpy(np.ascontiguousarray(scale, np.float32)).to(DEV)
    zt = torch.from_numpy(np.ascontiguousarray(zp, np.float32)).to(DEV)
    out = torch.empty_like(xt)
    lv = torch.empty(xt.shape, dtype={1: torch.int8, 2: torch.int16, 4: torch.int32}[lb], device=DEV)
    rc = lib.load().spq_fakequant(xt.data_ptr(), outer, chan, inner, st.data_ptr(), zt.data_ptr(), per_channel, bits,
                                  lib.QTYPE_ANY[qtype], 1 if sym else 0, out.data_ptr(), lv.data_ptr(), lb,
                                  lib.stream_ptr(xt.device))
    lib.check(rc, "spq_fakequant")
    torch.cuda.synchronize()
    return out.cpu().numpy(), lv.cpu().numpy().astype(np.float32)


FQ_CASES = [(b, "log") for b in (3, 4, 6, 8, 9, 12, 16, 24)] + [(6, "log_direct"), (18, "log_direct")]


def _level_bytes(bits, sym):
    top = (1 << (bits - 1)) - 1 if sym else (1 << bits) - 1
    return [lb for lb in (1, 2, 4) if lb == 4 or top <= (127 if lb == 1 else 32767)]


@pytest.mark.parametrize("bits,qtype", FQ_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_fakequant_levels_at_ties(pkg, bits, qtype, sym):
    direct = qtype == "log_direct"
    X, mins, ranges, _ = L.tie_matrix(bits, sym, 80, seed=bits + 100 * sym)
    rows = X.shape[0] - X.shape[0] % 4
    X = np.ascontiguousarray(X[:rows])
    q_ref, o_ref, amb = _expect(X, mins[None], ranges[None], bits, sym, direct)
    _check_coverage(X, mins[None], ranges[None], bits, sym, what=f"fakequant {bits}-bit {qtype} sym={sym}")
    print(f"  ambiguous (excluded): {int(amb.sum())}")
    for lb in _level_bytes(bits, sym):
        # MODE 1: x [rows, chan], one scale per column
        o, q = _fakequant(pkg, X, rows, 80, 1, ranges, mins, 1, bits, qtype, sym, lb)
        _assert_levels(q, q_ref, amb, f"mode 1 int{8 * lb}")
        _assert_dequant(o, o_ref, amb, f"mode 1 int{8 * lb}")
        # MODE 2: x^T [chan, rows], rows % 4 == 0
        o, q = _fakequant(pkg, np.ascontiguousarray(X.T), 1, 80, rows, ranges, mins, 1, bits, qtype, sym, lb)
        _assert_levels(q.T, q_ref, amb, f"mode 2 int{8 * lb}")
        _assert_dequant(o.T, o_ref, amb, f"mode 2 int{8 * lb}")
        # MODE 0: 79 channels (chan % 4 != 0)
        Xr = np.ascontiguousarray(X[:, :79])
        o, q = _fakequant(pkg, Xr, rows, 79, 1, ranges[:79], mins[:79], 1, bits, qtype, sym, lb)
        _assert_levels(q, q_ref[:, :79], amb[:, :79], f"mode 0 int{8 * lb}")
        _assert_dequant(o, o_ref[:, :79], amb[:, :79], f"mode 0 int{8 * lb}")


@pytest.mark.parametrize("bits", [4, 8, 16])
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_fakequant_per_tensor_at_ties(pkg, bits, sym):
    """One quantizer for the whole tensor (MODE 2 with per_channel = 0): the ties of every region under one (log_min, log_range)."""
    m, R = np.float32(-6.0), np.float32(12.0)
    x = np.concatenate([L.tie_inputs(m, R, bits, sym, r, span=24, max_ties=64, seed=i) for i, r in enumerate(L.REGIONS)])
    x = np.resize(x, (len(x) + 3) // 4 * 4).astype(np.float32)
    q_ref, o_ref, amb = _expect(x, m, R, bits, sym, False)
    _check_coverage(x, m, R, bits, sym, what=f"per-tensor {bits}-bit sym={sym}")
    o, q = _fakequant(pkg, x, 1, 1, len(x), np.array([R]), np.array([m]), 0, bits, "log", sym, 4)
    _assert_levels(q, q_ref, amb, "per-tensor")
    _assert_dequant(o, o_ref, amb, "per-tensor")


# ---- fakequant_transposed_kernel (LoRA-A): out[c, r] = FQ(x)[r, c] ------------------------------------------------------------
@pytest.mark.parametrize("bits,qtype", [(4, "log"), (8, "log"), (12, "log"), (16, "log"), (6, "log_direct")], ids=lambda v: str(v))
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_transposed_fakequant_at_ties(pkg, bits, qtype, sym):
    """Only dequantised values come out: within 1 ulp of the correctly rounded chain.  Wherever the neighbouring levels
    dequantise more than 2 ulps away (all but the narrowest ranges), that pins the level too; the coverage counts only those."""
    direct = qtype == "log_direct"
    X, mins, ranges, _ = L.tie_matrix(bits, sym, 72, seed=bits + 7)
    q_ref, o_ref, amb = _expect(X, mins[None], ranges[None], bits, sym, direct)
    _, qlo, qhi = L.level_range(bits, sym)
    sep = np.ones(X.shape, bool)
    for dq in (-1, 1):
        qn = np.clip(q_ref + dq, qlo, qhi)
        o_n = L.dequant(X, qn, mins[None], ranges[None], bits, sym, direct)
        sep &= (qn == q_ref) | (L.ulp_distance(o_n, o_ref) > 2)
    _check_coverage(X, mins[None], ranges[None], bits, sym, mask=sep, what=f"transposed {bits}-bit {qtype} sym={sym}")
    rows, cols = X.shape
    lib = pkg._lib
    xt = torch.from_numpy(X).to(DEV)
    st, zt = torch.from_numpy(ranges).to(DEV), torch.from_numpy(mins).to(DEV)
    out = torch.empty((cols, rows), dtype=torch.float32, device=DEV)
    rc = lib.load().spq_fakequant_transposed(xt.data_ptr(), rows, cols, st.data_ptr(), zt.data_ptr(), 1, bits,
                                             lib.QTYPE_ANY[qtype], 1 if sym else 0, 1.0, out.data_ptr(), lib.stream_ptr(xt.device))
    lib.check(rc, "spq_fakequant_transposed")
    o = out.cpu().numpy().T
    _assert_dequant(o, o_ref, amb, "transposed")


# ---- calibration statistics (stats_merge_kernel, log domain) -------------------------------------------------------------------
@pytest.mark.parametrize("per_channel", [True, False], ids=["per_channel", "per_tensor"])
def test_log_statistics_are_the_correctly_rounded_log2(pkg, per_channel):
    """running_min / running_max = float32(log2(float64(max(min|x|, eps)))) of the batches' own extremes, bit for bit, and
    zero_point / scale after finish_calibration follow from them exactly (log_min, log_max - log_min)."""
    rng = np.random.default_rng(3)
    q = pkg.LearnableFakeQuantize(8, channel_dim=-1, quantizer_type="log", per_channel=per_channel).to(DEV)
    q.start_calibration()
    batches = []
    for b in range(4):
        X, _, _, _ = L.tie_matrix(8, True, 96, seed=b)
        X = X[: 256 + 37 * b]
        X = X * np.exp2(rng.integers(-20, 20, (1, 96))).astype(np.float32)   # extremes spread over many binades
        if b == 2:
            X[:, 5] = 0.0                                                     # a channel at the clamp in one batch
        batches.append(X)
        q(torch.from_numpy(X).to(DEV))
    tmin = q.temp_min.detach().cpu().numpy().reshape(-1)
    tmax = q.temp_max.detach().cpu().numpy().reshape(-1)
    q.finish_calibration()
    ax = np.abs(np.concatenate(batches))
    lo = ax.min(axis=0) if per_channel else ax.min(keepdims=True).reshape(1)
    hi = ax.max(axis=0) if per_channel else ax.max(keepdims=True).reshape(1)
    lo64, hi64 = (np.log2(np.maximum(v, L.EPS).astype(np.float64)) for v in (lo, hi))
    amb = L.ambiguous_lg(lo64, 0, 1, 8, True) | L.ambiguous_lg(hi64, 0, 1, 8, True)
    print(f"statistics: {lo.size} channels, {int(amb.sum())} ambiguous")
    ok = ~amb
    np.testing.assert_array_equal(tmin[ok], lo64.astype(np.float32)[ok])
    np.testing.assert_array_equal(tmax[ok], hi64.astype(np.float32)[ok])
    rmin = q.running_min.cpu().numpy().reshape(-1)
    rmax = q.running_max.cpu().numpy().reshape(-1)
    np.testing.assert_array_equal(rmin, tmin)
    np.testing.assert_array_equal(rmax, tmax)
    np.testing.assert_array_equal(q.zero_point.cpu().numpy().reshape(-1), rmin)
    np.testing.assert_array_equal(q.scale.cpu().numpy().reshape(-1), (rmax - rmin).astype(np.float32))


# ---- the activation pass of the fused forward (streaming limb form, panel kernels) ---------------------------------------------
def _identity_layer(pkg, K, bits, sym, mins, ranges):
    """SPLinearWithLoRA with W = I, B = 0: y[m, k] = FQ(x)[m, k] * c_k, and with the weight quantizer's log_min = log_range = 0
    c_k = FQ(1) = 2^0 = 1 exactly (off-diagonal zeros dequantise to 0 by the zero mask)."""
    r = 64
    layer = pkg.SPLinearWithLoRA(K, K, [bits, 32], {bits: r, 32: 0}, {bits: r, 32: 0}, {bits: "log", 32: None})
    key = f"{bits}bit"
    lora = layer.lora_adapters[key]
    with torch.no_grad():
        layer.linear.weight.copy_(torch.eye(K))
        layer.linear.bias.zero_()
        lora.lora_A.copy_(torch.randn(K, r, generator=torch.Generator().manual_seed(1)) * 0.1)
        lora.lora_B.zero_()
    layer = layer.to(DEV).eval()
    layer.set_precision(bits)
    key_q = (layer.quantizers_input[key], layer.quantizers_weight[key], lora.quantize_A, lora.quantize_B)
    for qq in key_q:
        qq.symmetric = sym
        qq._update_quant_range()
    calib = torch.from_numpy(np.exp2(np.linspace(-4, 4, 4 * K, dtype=np.float32)).reshape(4, K)).to(DEV)
    pkg.calibrate_layer(layer, bits, [calib])
    qx, qw = key_q[0], key_q[1]
    with torch.no_grad():
        qx.zero_point.copy_(torch.from_numpy(mins).reshape(qx.zero_point.shape))
        qx.scale.copy_(torch.from_numpy(ranges).reshape(qx.scale.shape))
        qw.zero_point.zero_()
        qw.scale.zero_()
        qx._epoch += 1
        qw._epoch += 1
    layer.invalidate_operand_cache()
    return layer


ACT_CASES = [  # K, bits, sym, M
    (128, 4, True, 2048), (128, 6, False, 2048), (128, 8, True, 16400), (128, 12, True, 2048), (128, 16, False, 16400),
]


@pytest.mark.parametrize("case", ACT_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_activation_pass_levels_at_ties(pkg, case):
    import os
    K, bits, sym, M = case
    X, mins, ranges, _ = L.tie_matrix(bits, sym, K, regions=("R1", "R4", "R2"), seed=bits + K)
    X = np.resize(X, (M, K)) if X.shape[0] < M else X[:M]
    X = np.ascontiguousarray(X, np.float32)
    q_ref, o_ref, amb = _expect(X, mins[None], ranges[None], bits, sym, False)
    # the limb form carries FQ(x) as two f16 pieces under one power-of-two scale per tensor: ~2^-21 relative, and an absolute floor
    # far below the tensor's largest value.  An element is decodable where its neighbouring levels dequantise further than twice
    # that from it
    tol = np.abs(o_ref) * 2.0 ** -20 + np.abs(o_ref).max() * 2.0 ** -36
    _, qlo, qhi = L.level_range(bits, sym)
    sep = np.ones(X.shape, bool)
    for dq in (-1, 1):
        qn = np.clip(q_ref + dq, qlo, qhi)
        o_n = L.dequant(X, qn, mins[None], ranges[None], bits, sym, False)
        sep &= (qn == q_ref) | (np.abs(o_n - o_ref) > 2 * tol)
    _check_coverage(X, mins[None], ranges[None], bits, sym, mask=sep, what=f"activation pass {case}")
    layer = _identity_layer(pkg, K, bits, sym, mins, ranges)
    xt = torch.from_numpy(X).to(DEV)
    saved = {k: os.environ.get(k) for k in ("SPQ_XPASS_STREAM", "SPQ_XPASS_STREAM_LIMBS")}
    try:
        for name, sw in (("default", {}), ("panel limbs", {"SPQ_XPASS_STREAM_LIMBS": "0"}),
                         ("panel", {"SPQ_XPASS_STREAM": "0"})):
            for k in saved:
                pkg._lib.set_switch(k, sw.get(k, saved[k]))
            with torch.no_grad():
                y = layer(xt).cpu().numpy()
            assert y.shape == o_ref.shape and not np.isnan(y).any(), \
                f"{name}: {int(np.isnan(y).sum())} NaN in y, first at {np.argwhere(np.isnan(y))[:4].tolist()}"
            err = np.where(amb, 0, np.abs(y - o_ref))
            r = err / tol
            i = np.unravel_index(np.argmax(r), r.shape)
            assert r[i] <= 1.0, (f"{name}: |y - FQ_exact(x)| reaches {r[i]:.3g} x the limb bound (a level moved) at {i}: "
                                 f"x {X[i]!r} y {y[i]!r} exact {o_ref[i]!r} level {q_ref[i]}")
    finally:
        for k, v in saved.items():
            pkg._lib.set_switch(k, v)
