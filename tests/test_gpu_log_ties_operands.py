"""Log levels at the rounding ties at the operand sites: weight preparation, LoRA-A / LoRA-B, part2's W_eff and factors, and the
levels-out store of the fused forward -- against the correctly rounded chain (tests/log_exact.py).

Each of these sites is its own inlined instance of fq_dispatch / log_level (spq_f16x2.hip), so a wrong error bound or a missing
fp64 fallback at one of them is invisible to test_gpu_log_ties.py.  The inputs are built on and around the ties; levels must be
those of the exact chain outside log_exact's ambiguity mask (reported).  Values read back in fp32 must be within 1 ulp of the
correctly rounded dequantisation.  Values read back as two fp16 limbs (log_exact.split2) are decoded, and there a level is
decided only where the neighbouring levels dequantise more than twice the limb tolerance away (log_exact.separable).  Every
case asserts its coverage on what it can decode: MIN_EXACT elements exactly on k + 1/2 and MIN_NEAR within the device's bound."""
import ctypes
import os

import numpy as np
import pytest
import torch

import log_exact as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIN_EXACT, MIN_NEAR = 100, 1000
A_SENTINEL = 5.0


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    return p


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _coverage(x, mins, ranges, bits, sym, mask, what):
    exact, near = L.coverage(np.where(mask, x, np.float32(np.nan)), mins, ranges, bits, sym)
    print(f"{what}: {exact} on k+1/2, {near} within the device bound, {int(mask.size - mask.sum())} not decodable")
    assert exact >= MIN_EXACT and near >= MIN_NEAR, (what, exact, near)


def _assert_within(got, ref, tol, amb, what):
    err = np.where(amb, 0.0, np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)))
    r = err / tol
    i = np.unravel_index(np.argmax(r), r.shape)
    assert r[i] <= 1.0, f"{what}: read-back off by {r[i]:.3g} x the limb tolerance (a level moved) at {i}: got {got[i]!r} exact {ref[i]!r}"


def _assert_ulp(got, ref, amb, what):
    d = np.where(amb, 0, L.ulp_distance(got, ref))
    i = np.unravel_index(np.argmax(d), d.shape)
    assert int(d[i]) <= 1, f"{what}: {int(d[i])} ulp from the correctly rounded chain at {i}: got {got[i]!r} exact {ref[i]!r}"


def _case(X, mins, ranges, bits, sym, direct, what):
    """The exact chain of a per-column tie matrix: levels, dequantised values, ambiguity mask (count printed)."""
    q = L.levels(X, mins, ranges, bits, sym)
    o = L.dequant(X, q, mins, ranges, bits, sym, direct)
    amb = L.ambiguous(X, mins, ranges, bits, sym)
    print(f"{what}: {int(amb.sum())} ambiguous (excluded)")
    return q, o, amb


# ---- weight preparation: prep_wave_kernel<0,4> / <0,16>, prep_f16x2_kernel; LoRA-A in the same grid -------------------------------
class _Prep:
    """The arguments of one weight preparation (spq_prepare_args) with their device tensors and output buffers.
    wq / bq / aq = (scale, zero, per_channel, bits, qtype, sym); B / A may be None."""

    def __init__(self, pkg, W, N, K, wq, B, r, bq, scaling, A, aq, sx, x_pc, path):
        lib = pkg._lib.load()
        self.N, self.K, self.r = N, K, r
        self.Np, self.Kp, self.Rp = -(-N // 128) * 128, -(-K // 64) * 64, (-(-r // 64) * 64 if r else 0)
        self.nbytes = lib.spq_prep_f16x2_bytes(N, K, r)
        self.wp = torch.full((self.nbytes // 2 + 8,), 7.0, dtype=torch.float16, device=DEV)   # padding must be written
        self.rs = torch.full((self.Np,), 3.0, dtype=torch.float32, device=DEV)
        # FQ(A)^T: rows >= r belong to the caller (zeroed there) and must not be written -- a sentinel shows that they were not
        self.ap = torch.full((-(-r // 64) * 64, K), A_SENTINEL, dtype=torch.float32, device=DEV) if A is not None else None
        t = lambda a: _t(a) if a is not None else None
        self.keep = [t(W), t(B), t(A), t(wq[0]), t(wq[1]), t(sx)] + ([t(bq[0]), t(bq[1])] if B is not None else [None, None]) \
            + ([t(aq[0]), t(aq[1])] if A is not None else [None, None])
        Wt, Bt, At, ws, wz, sxt, bs, bz, a_s, a_z = self.keep
        pp = lambda x: x.data_ptr() if x is not None else None
        Q = pkg._lib.QTYPE_ANY
        self.args = pkg._lib.PrepareArgs(
            W=Wt.data_ptr(), N=N, K=K, sw=ws.data_ptr(), zw=wz.data_ptr(), w_per_channel=wq[2], w_bits=wq[3],
            w_qtype=Q[wq[4]], w_symmetric=int(wq[5]),
            B=pp(Bt), r=r, sb=pp(bs), zb=pp(bz), b_per_channel=bq[2] if B is not None else 0, b_bits=bq[3] if B is not None else 0,
            b_qtype=Q[bq[4]] if B is not None else 0, b_symmetric=int(bq[5]) if B is not None else 1, scaling=scaling,
            A=pp(At), sa=pp(a_s), za=pp(a_z), a_per_channel=aq[2] if A is not None else 0, a_bits=aq[3] if A is not None else 0,
            a_qtype=Q[aq[4]] if A is not None else 0, a_symmetric=int(aq[5]) if A is not None else 1,
            sx=sxt.data_ptr(), x_per_channel=x_pc, w_prep=self.wp.data_ptr(), w_prep_bytes=self.nbytes,
            w_rowscale=self.rs.data_ptr(), a_prep=pp(self.ap), path=path)

    def run(self, pkg):
        rc = pkg._lib.load().spq_prepare_f16x2_args(ctypes.byref(self.args), pkg._lib.stream_ptr(DEV))
        pkg._lib.check(rc, "spq_prepare_f16x2")
        return self.read()

    def read(self):
        """(Whi, Wlo, Bhi, Blo) as numpy float16 [Np, Kp] / [Np, Rp] (make_prep_layout), rowscale [Np], a_prep, raw bytes."""
        torch.cuda.synchronize()
        raw = self.wp.cpu().numpy().view(np.uint8)[:self.nbytes]
        o, planes = 0, []
        for rows, cols in ((self.Np, self.Kp), (self.Np, self.Kp), (self.Np, self.Rp), (self.Np, self.Rp)):
            planes.append(raw[o:o + rows * cols * 2].view(np.float16).reshape(rows, cols))
            o += -(-(rows * cols * 2) // 256) * 256
        return planes, self.rs.cpu().numpy(), (self.ap.cpu().numpy() if self.ap is not None else None), raw.copy()


def _prepare(pkg, W, N, K, wq, B, r, bq, scaling, A, aq, sx, x_pc, path=2):
    return _Prep(pkg, W, N, K, wq, B, r, bq, scaling, A, aq, sx, x_pc, path).run(pkg)[:3]


def _check_padding(planes, rs, N, K, r, what):
    whi, wlo, bhi, blo = planes
    assert not whi[N:].any() and not wlo[N:].any() and not whi[:, K:].any() and not wlo[:, K:].any(), f"{what}: W padding not zero"
    if r:
        assert not bhi[N:].any() and not blo[N:].any() and not bhi[:, r:].any() and not blo[:, r:].any(), f"{what}: B padding not zero"
    assert (rs[N:] == 1.0).all(), f"{what}: padding rows' scale is not 1"


def _check_a_prep(ap, A, amins, aranges, bits, sym, direct, r, what):
    """a_prep rows 0..r-1 = FQ(A)^T within 1 ulp; coverage on what 1 ulp pins; the rows past r are left as the caller had them."""
    qa, oa, amba = _case(A, amins[None], aranges[None], bits, sym, direct, what)
    sep = L.separable(A, qa, oa, amins[None], aranges[None], bits, sym, direct)
    _coverage(A, amins[None], aranges[None], bits, sym, sep, what)
    _assert_ulp(ap[:r].T, oa, amba, what)
    assert (ap[r:] == A_SENTINEL).all(), f"{what}: rows of FQ(A)^T past r were written"


# K, N, r, bits, qtype, sym, per-channel power-of-two input scale.  K = 768: prep_wave_kernel<0,4>; K = 3072: <0,16>;
# K = 1030 (K % 4 != 0) and K = 4160 (> 4096): prep_f16x2_kernel.  N % 128 != 0 everywhere (padding rows).
PREP_CASES = [
    (768, 200, 64, 4, "log", True, False),
    (768, 136, 100, 8, "log", False, True),
    (768, 200, 48, 12, "log", True, False),
    (3072, 136, 128, 6, "log_direct", True, False),
    (3072, 200, 64, 16, "log", False, True),
    (1030, 200, 100, 16, "log", True, False),
    (1030, 136, 64, 3, "log", False, True),
    (4160, 136, 32, 9, "log_direct", False, False),
]


def prep_weight_inputs(K, N, r, bits, sym, x_pc, seed):
    """W [N, K] with a tie quantizer per output row (tie_matrix transposed), A [K, r] with one per column, the input scale."""
    X, wm, wr, _ = L.tie_matrix(bits, sym, N, rows=K, seed=seed)
    A, am, ar, _ = L.tie_matrix(bits, sym, r, rows=K, seed=seed + 1)
    sx = np.exp2(np.random.default_rng(seed).integers(-3, 4, K)).astype(np.float32) if x_pc else np.ones(1, np.float32)
    return np.ascontiguousarray(X.T), wm, wr, np.ascontiguousarray(A), am, ar, sx


def prep_weight_expect(W, wm, wr, bits, sym, direct, sx, rowscale):
    q, o, amb = _case(W, wm[:, None], wr[:, None], bits, sym, direct, "W")
    ref = (o * sx[None, :]).astype(np.float32)                    # W' = fl32(FQ(W) * sx): exact for a power-of-two sx
    tol = L.limb_tol(ref, rowscale[:, None])
    sep = L.separable(W, q, ref, wm[:, None], wr[:, None], bits, sym, direct, tol=tol, scale=sx[None, :])
    return ref, tol, sep, amb


@pytest.mark.parametrize("case", PREP_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_weight_prep_levels_at_ties(pkg, case):
    K, N, r, bits, qtype, sym, x_pc = case
    direct = qtype == "log_direct"
    seed = K + bits
    W, wm, wr, A, am, ar, sx = prep_weight_inputs(K, N, r, bits, sym, x_pc, seed)
    B = np.zeros((r, N), np.float32)                               # FQ(0) = 0: B' = 0 leaves the row scale to W'
    wq = (wr, wm, 1, bits, qtype, sym)
    bq = (np.full(N, 8.0, np.float32), np.full(N, -4.0, np.float32), 1, bits, qtype, sym)
    aq = (ar, am, 1, bits, qtype, sym)
    planes, rs, ap = _prepare(pkg, W, N, K, wq, B, r, bq, 0.5, A, aq, sx, int(x_pc))
    _check_padding(planes, rs, N, K, r, "weight prep")
    assert not planes[2].any() and not planes[3].any(), "B' of B = 0 is not zero"
    ref, tol, sep, amb = prep_weight_expect(W, wm, wr, bits, sym, direct, np.broadcast_to(sx, (K,)), rs[:N])
    _coverage(W, wm[:, None], wr[:, None], bits, sym, sep, f"W' limbs {case}")
    got = L.limb_decode(planes[0][:N, :K], planes[1][:N, :K], rs[:N, None])
    _assert_within(got, ref, tol, amb, "W' limbs")
    _check_a_prep(ap, A, am, ar, bits, sym, direct, r, f"LoRA-A in the prep grid {case}")


def _check_lora_b(planes, rs, B, bm, br, bits, sym, direct, scaling, what):
    """Bhi/Blo [Np, Rp] decoded with the row scales: scaling * FQ(B)[:, n] of B [r, N] (one quantizer per output row n)."""
    r, N = B.shape
    q, o, amb = _case(B, bm[None], br[None], bits, sym, direct, what)
    ref = (o * np.float32(scaling)).T
    tol = L.limb_tol(ref, rs[:N, None])
    sep = L.separable(B, q, o * np.float32(scaling), bm[None], br[None], bits, sym, direct, tol=tol.T, scale=scaling)
    _coverage(B, bm[None], br[None], bits, sym, sep, what)
    got = L.limb_decode(planes[2][:N, :r], planes[3][:N, :r], rs[:N, None])
    _assert_within(got, ref, tol, amb.T, what)


@pytest.mark.parametrize("case", PREP_CASES[::2] + PREP_CASES[5:6], ids=lambda c: "-".join(str(v) for v in c))
def test_lora_b_prep_levels_at_ties(pkg, case):
    """B' = scaling * FQ(B)[:, n] shares the row scale with W'; W = 0 (FQ(0) = 0) so that B alone sets it."""
    K, N, r, bits, qtype, sym, _ = case
    direct = qtype == "log_direct"
    B, bm, br, _ = L.tie_matrix(bits, sym, N, rows=r, seed=r + bits)          # [r, N]: one quantizer per output row n
    W = np.zeros((N, K), np.float32)
    wq = (np.ones(1, np.float32), np.zeros(1, np.float32), 0, 8, "minmax", True)
    scaling = 2.0 if bits % 2 else 0.25
    planes, rs, _ = _prepare(pkg, W, N, K, wq, B, r, (br, bm, 1, bits, qtype, sym), scaling, None, None,
                             np.ones(1, np.float32), 0)
    _check_padding(planes, rs, N, K, r, "LoRA-B prep")
    assert not planes[0].any() and not planes[1].any(), "W' of W = 0 is not zero"
    _check_lora_b(planes, rs, B, bm, br, bits, sym, direct, scaling, f"B' limbs {case}")


# ---- the same rows inside the activation launch: xpass_stream_prep_kernel (SPQ_PREP_ROLE) and fq_transpose_kernel -----------------
def _device_kernels(fn):
    """Names of the GPU kernels that fn() launched (torch.profiler's device activity: every dispatch of the process)."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return {e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA}


@pytest.mark.parametrize("operand", ["W", "B"])
@pytest.mark.parametrize("xq", ["minmax", "log"])
def test_role_fused_prepare_at_ties(pkg, xq, operand):
    """spq_fwd_args.prepare on a shape whose row work rides in the streaming activation launch (K % 64 == 0, K <= 1024, r <= 64,
    no LayerNorm): w_prep, the row scales and FQ(A)^T must be the bytes of the preparation launch, and decode to the exact chain.
    A min-max input takes the f16x2 path (A8 = 0), a log input the two-limb one (A8 = 3).  The ties are in W (B = 0) or in B
    (W = 0), as in the preparation tests; FQ(A)^T (fq_transpose_kernel) is at the ties in both.  The launch is traced, so that a
    quiet fall-back to the preparation launch cannot pass."""
    lib = pkg._lib.load()
    M, K, N, r, bits, qtype, sym = 512, 768, 200, 64, 8, "log", True
    W, wm, wr, A, am, ar, _ = prep_weight_inputs(K, N, r, bits, sym, False, seed=77)
    wq, aq = (wr, wm, 1, bits, qtype, sym), (ar, am, 1, bits, qtype, sym)
    if operand == "W":
        B = np.zeros((r, N), np.float32)
        bq = (np.full(N, 8.0, np.float32), np.full(N, -4.0, np.float32), 1, bits, qtype, sym)
    else:
        B, bm, br, _ = L.tie_matrix(bits, sym, N, rows=r, seed=78)
        bq = (br, bm, 1, bits, qtype, sym)
        W = np.zeros((N, K), np.float32)
        wq = (np.ones(1, np.float32), np.zeros(1, np.float32), 0, 8, "minmax", True)
    if xq == "minmax":
        path, sx, zx, limb = pkg._lib.PATH_F16X2, np.full(1, 0.25, np.float32), np.zeros(1, np.float32), None
    else:
        path, sx, zx, limb = pkg._lib.PATH_F16X3, np.full(1, 8.0, np.float32), np.full(1, -4.0, np.float32), _pow2(9)
    sx_prep = sx if xq == "minmax" else np.ones(1, np.float32)     # no scale folding on the two-limb path
    ref = _Prep(pkg, W, N, K, wq, B, r, bq, 0.5, A, aq, sx_prep, 0, path).run(pkg)
    role = _Prep(pkg, W, N, K, wq, B, r, bq, 0.5, A, aq, sx_prep, 0, path)
    x = _t(np.random.default_rng(5).standard_normal((M, K)))
    sxt, zxt, lt = _t(sx), _t(zx), _t(limb) if limb is not None else None
    y = torch.empty(M, N, dtype=torch.float32, device=DEV)
    need = lib.spq_fwd_workspace_bytes(M, K, N, r, path)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    args = pkg._lib.FwdArgs(
        M=M, K=K, N=N, r=r, bits=4 if xq == "minmax" else 6, qtype=pkg._lib.QTYPE_CODE[xq], symmetric=1, quantize_input=1,
        x_per_channel=0, path=path, x=x.data_ptr(), sx=sxt.data_ptr(), zx=zxt.data_ptr(),
        x_limb_scale=lt.data_ptr() if lt is not None else None, w_prep=role.wp.data_ptr(), w_rowscale=role.rs.data_ptr(),
        a_prep=role.ap.data_ptr(), b_prep=role.wp.data_ptr(), lora_scaling=0.5, y=y.data_ptr(), workspace=ws.data_ptr(),
        workspace_bytes=need, stage=pkg._lib.STAGE_ALL, epilogue=pkg._lib.EPILOGUE_NONE)
    args.prepare = ctypes.pointer(role.args)
    saved = {k: os.environ.get(k) for k in ("SPQ_XPASS_STREAM", "SPQ_XPASS_STREAM_LIMBS", "SPQ_PREP_ROLE")}
    try:
        for k in saved:
            pkg._lib.set_switch(k, None)
        def fwd():
            pkg._lib.check(lib.spq_linear_lora_fwd(ctypes.byref(args), pkg._lib.stream_ptr(DEV)), "spq_linear_lora_fwd(prepare)")
        names = _device_kernels(fwd)
    finally:
        for k, v in saved.items():
            pkg._lib.set_switch(k, v)
    planes, rs, ap, raw = role.read()
    print(f"role-fused ({xq} input) launched: {sorted(names)}")
    for k in ("xpass_stream_prep_kernel", "fq_transpose_kernel"):
        assert any(k in n for n in names), f"{k} did not run: {sorted(names)}"
    assert not any("prep_wave_kernel" in n or "prep_f16x2_kernel" in n for n in names), "the preparation launch ran instead"
    assert np.array_equal(raw, ref[3]), f"role-fused w_prep differs from the preparation launch in {int((raw != ref[3]).sum())} bytes"
    assert np.array_equal(rs, ref[1]) and np.array_equal(ap, ref[2])
    if operand == "W":          # (with B at the ties too, x . FQ(A) . FQ(B) overflows fp32: both hold |lg| ~ 120 ties)
        assert bool(torch.isfinite(y).all())
    _check_padding(planes, rs, N, K, r, "role-fused prep")
    if operand == "W":
        ref_w, tol, sep, amb = prep_weight_expect(W, wm, wr, bits, sym, False, np.ones(K, np.float32) * sx_prep[0], rs[:N])
        _coverage(W, wm[:, None], wr[:, None], bits, sym, sep, f"role-fused W' limbs ({xq} input)")
        _assert_within(L.limb_decode(planes[0][:N, :K], planes[1][:N, :K], rs[:N, None]), ref_w, tol, amb, "role-fused W' limbs")
    else:
        assert not planes[0].any() and not planes[1].any(), "W' of W = 0 is not zero"
        _check_lora_b(planes, rs, B, bm, br, bits, sym, False, 0.5, f"role-fused B' limbs ({xq} input)")
    _check_a_prep(ap, A, am, ar, bits, sym, False, r, f"LoRA-A through fq_transpose_kernel ({xq} input)")


# ---- the LayerNorm prologue of the activation pass (xpass_stream_kernel<R, 3, true>, ln_panel_apply) -----------------------------
LN_CASES = [(128, 4, True), (128, 8, False), (256, 12, True), (128, 16, False), (128, 6, True)]   # K, bits, sym


@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_layernorm_prologue_levels_at_ties(pkg, case):
    """layer(x, pre_norm=ln) with a log input quantizer normalises inside the activation pass.  ln.bias[k] sits on a tie of
    column k and ln.weight[k] is a few ulps of it (log_exact.ln_ties), so weight * n + bias lands on and around the ties.  The
    prologue must give the bits of spq_layernorm (the unfused layer on ln(x) is bit-identical), and y = FQ(ln(x)) through the
    identity weight must decode to the exact chain's levels on that spq_layernorm output -- streaming kernel and panel kernel."""
    from test_gpu_log_ties import _identity_layer
    K, bits, sym = case
    M = 2048
    x, w, b, mins, ranges = L.ln_ties(bits, sym, K, M, seed=K + bits, max_lg=20.0)
    layer = _identity_layer(pkg, K, bits, sym, mins, ranges)
    ln = pkg.SwitchableLayerNorm(K, [bits, 32]).to(DEV)
    with torch.no_grad():
        ln.weights[str(bits)].copy_(torch.from_numpy(w))
        ln.biases[str(bits)].copy_(torch.from_numpy(b))
    ln.set_precision(bits)
    xt = _t(x)
    with torch.no_grad():
        n_t = ln(xt)                                                  # spq_layernorm
    n = n_t.cpu().numpy()
    tag = f"LayerNorm prologue {case}"
    q, o, amb = _case(n, mins[None], ranges[None], bits, sym, False, tag)
    tol = np.abs(o) * 2.0 ** -20 + np.exp2(np.max(mins.astype(np.float64) + ranges)) * 2.0 ** -36   # the limb form's bound
    sep = L.separable(n, q, o, mins[None], ranges[None], bits, sym, tol=tol)
    _coverage(n, mins[None], ranges[None], bits, sym, sep, tag)
    saved = {k: os.environ.get(k) for k in ("SPQ_XPASS_STREAM", "SPQ_XPASS_STREAM_LIMBS")}
    try:
        for name, sw in (("streaming", {"SPQ_XPASS_STREAM": None, "SPQ_XPASS_STREAM_LIMBS": None}),
                         ("panel", {"SPQ_XPASS_STREAM": "0", "SPQ_XPASS_STREAM_LIMBS": None})):
            for k, v in sw.items():
                pkg._lib.set_switch(k, v)
            with torch.no_grad():
                names = _device_kernels(lambda: layer(xt, pre_norm=ln))
                assert layer._norm_fused, f"{name}: the LayerNorm was not fused into the activation pass"
                y_f = layer(xt, pre_norm=ln)
                assert layer._norm_fused
                y_u = layer(n_t)                                      # the same layer on spq_layernorm's output
            want = "xpass_stream_kernel" if name == "streaming" else "xpass_panel_kernel"
            assert any(want in k for k in names), f"{name}: {want} did not run: {sorted(names)}"
            assert torch.equal(y_f, y_u), f"{name}: the prologue differs from spq_layernorm"
            _assert_within(y_f.cpu().numpy(), o, tol, amb, f"{tag} {name}")
    finally:
        for k, v in saved.items():
            pkg._lib.set_switch(k, v)


# ---- part2: cpt_factors_kernel, cpt_weff_kernel (spq_prepare_cpt, path F32) -------------------------------------------------------
def _prepare_cpt(pkg, W, N, K, wq, A, B, r, lq, scaling):
    lib = pkg._lib.load()
    Wt, At, Bt = _t(W), _t(A), _t(B)
    ws, wz, ls, lz = _t(wq[0]), _t(wq[1]), _t(lq[0]), _t(lq[1])
    w_eff = torch.empty(N, K, dtype=torch.float32, device=DEV)
    aq = torch.empty(K, r, dtype=torch.float32, device=DEV)
    bq = torch.empty(N, r, dtype=torch.float32, device=DEV)
    aq_t = torch.full((-(-r // 64) * 64, K), 5.0, dtype=torch.float32, device=DEV)
    Q = pkg._lib.QTYPE_ANY
    rc = lib.spq_prepare_cpt(Wt.data_ptr(), N, K, ws.data_ptr(), wz.data_ptr(), wq[2], wq[3], Q[wq[4]], int(wq[5]),
                             At.data_ptr(), Bt.data_ptr(), r, ls.data_ptr(), lz.data_ptr(), lq[2], lq[3], Q[lq[4]], int(lq[5]),
                             scaling, None, 0, pkg._lib.PATH_F32, None, 0, None, w_eff.data_ptr(), aq.data_ptr(), bq.data_ptr(),
                             aq_t.data_ptr(), pkg._lib.stream_ptr(DEV))
    pkg._lib.check(rc, "spq_prepare_cpt")
    torch.cuda.synchronize()
    return w_eff.cpu().numpy(), aq.cpu().numpy(), bq.cpu().numpy(), aq_t.cpu().numpy()


def cpt_inputs(N, K, r, bits, sym, per_channel, seed):
    """W [N, K] (a quantizer per row), and A [K, r] / B [N, r] sharing one quantizer per column j -- or, per tensor, every
    region's ties under one (log_min, log_range)."""
    if per_channel:
        X, wm, wr, _ = L.tie_matrix(bits, sym, N, rows=K, seed=seed)
        AB, lm, lr, _ = L.tie_matrix(bits, sym, r, rows=K + N, seed=seed + 1)
        return np.ascontiguousarray(X.T), wm, wr, np.ascontiguousarray(AB[:K]), np.ascontiguousarray(AB[K:]), lm, lr
    rng = np.random.default_rng(seed)

    def pool(m, R, n):                                           # every region's ties of one quantizer, n of them
        x = np.concatenate([L.tie_inputs(m, R, bits, sym, g, span=24, max_ties=64, seed=seed + i) for i, g in enumerate(L.REGIONS)])
        return rng.permutation(np.resize(x, n)).astype(np.float32)
    wm, wr, lm, lr = np.float32(-6.0), np.float32(12.0), np.float32(-7.0), np.float32(16.0)
    one = lambda v: np.array([v], np.float32)
    AB = pool(lm, lr, (K + N) * r).reshape(K + N, r)
    return pool(wm, wr, N * K).reshape(N, K), one(wm), one(wr), AB[:K], AB[K:], one(lm), one(lr)


CPT_CASES = [(6, True, True), (18, False, True), (6, False, False), (18, True, False), (9, True, True)]   # bits, sym, per-channel


@pytest.mark.parametrize("bits,sym,per_channel", CPT_CASES, ids=lambda v: str(v))
def test_cpt_prepare_levels_at_ties(pkg, bits, sym, per_channel):
    N, K, r = 192, 320, 48
    W, wm, wr, A, B, lm, lr = cpt_inputs(N, K, r, bits, sym, per_channel, seed=bits + 3 * sym)
    wq = (wr, wm, int(per_channel), bits, "log_direct", sym)
    lq = (lr, lm, int(per_channel), bits, "log_direct", sym)
    wm_, wr_ = (wm[:, None], wr[:, None]) if per_channel else (wm, wr)
    tag = f"part2 {bits}-bit sym={sym} per_channel={per_channel}"
    # W_eff = FQ(W) + s FQ(B) FQ(A)^T with FQ(B) = 0: FQ(W) itself
    w_eff, aq, _, aq_t = _prepare_cpt(pkg, W, N, K, wq, A, np.zeros((N, r), np.float32), r, lq, 0.5)
    q, o, amb = _case(W, wm_, wr_, bits, sym, True, "W")
    _coverage(W, wm_, wr_, bits, sym, L.separable(W, q, o, wm_, wr_, bits, sym, True), f"{tag} W_eff")
    _assert_ulp(w_eff, o, amb, "W_eff")
    qa, oa, amba = _case(A, lm, lr, bits, sym, True, "A")
    _coverage(A, lm, lr, bits, sym, L.separable(A, qa, oa, lm, lr, bits, sym, True), f"{tag} FQ(A)")
    _assert_ulp(aq, oa, amba, "FQ(A)")
    _assert_ulp(aq_t[:r].T, oa, amba, "FQ(A)^T")
    assert not aq_t[r:].any(), "padding rows of FQ(A)^T not zero"
    # FQ(B), the same per-column quantizer
    _, _, bq, _ = _prepare_cpt(pkg, W, N, K, wq, A, B, r, lq, 0.5)
    qb, ob, ambb = _case(B, lm, lr, bits, sym, True, "B")
    _coverage(B, lm, lr, bits, sym, L.separable(B, qb, ob, lm, lr, bits, sym, True), f"{tag} FQ(B)")
    _assert_ulp(bq, ob, ambb, "FQ(B)")


# ---- the levels-out store (gemm_f16x2_t128_kernel<.., LV>) -----------------------------------------------------------------------
def _store_forward(pkg, bias, s, Q, epilogue, out):
    """The fused forward with W = I (symmetric 8-bit min-max weights, power-of-two scale: FQ(I) = I exactly), r = 0 and an
    8-bit per-channel input scale s: row m of x is (m - Q) * s, so y[m, n] = bias[n] + (m - Q) * s[n] (then the epilogue).
    `out` = (hi plane, lo plane or None, out_scale, out_zero, qtype code, bits, sym, limb scale or None).  Returns y."""
    lib = pkg._lib.load()
    N = K = bias.size
    qs = np.r_[np.arange(-Q, Q + 1), np.zeros(255 - 2 * Q)].astype(np.float32)   # 256 rows
    M = qs.size
    x = (qs[:, None] * s[None, :]).astype(np.float32)
    W = np.eye(N, dtype=np.float32)
    one = np.array([2.0 ** -6], np.float32)
    nbytes = lib.spq_prep_f16x2_bytes(N, K, 0)
    wp = torch.empty(nbytes // 4 + 4, dtype=torch.float32, device=DEV)
    rs = torch.empty(-(-N // 128) * 128, dtype=torch.float32, device=DEV)
    Wt, ot, zt, st = _t(W), _t(one), _t(np.zeros(1)), _t(s)
    rc = lib.spq_prepare_f16x2(Wt.data_ptr(), N, K, ot.data_ptr(), zt.data_ptr(), 0, 8, 0, 1, None, 0, None, None, 0, 0, 0, 1, 0.0,
                               None, None, None, 0, 0, 0, 1, st.data_ptr(), 1, wp.data_ptr(), nbytes, rs.data_ptr(), None,
                               pkg._lib.stream_ptr(DEV))
    pkg._lib.check(rc, "spq_prepare_f16x2(identity)")
    xt, bt, zx = _t(x), _t(bias), _t(np.zeros(N))
    y = torch.empty(M, N, dtype=torch.float32, device=DEV)
    need = lib.spq_fwd_workspace_bytes(M, K, N, 0, pkg._lib.PATH_F16X2)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    hi, lo, osc, oz, oq, obits, osym, olimb = out
    args = pkg._lib.FwdArgs(
        M=M, K=K, N=N, r=0, bits=8, qtype=pkg._lib.MINMAX, symmetric=1, quantize_input=1, x_per_channel=1,
        path=pkg._lib.PATH_F16X2, x=xt.data_ptr(), sx=st.data_ptr(), zx=zx.data_ptr(), w_prep=wp.data_ptr(),
        w_rowscale=rs.data_ptr(), bias=bt.data_ptr(), y=y.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=need,
        stage=pkg._lib.STAGE_ALL, epilogue=epilogue, out_levels=hi.data_ptr(), out_levels_ld=N, out_scale=osc.data_ptr(),
        out_scale_per_channel=1, out_bits=obits, out_levels_lo=lo.data_ptr() if lo is not None else None,
        out_zero=oz.data_ptr() if oz is not None else None, out_qtype=oq, out_symmetric=1 if osym else 0,
        out_limb_scale=olimb.data_ptr() if olimb is not None else None)
    rc = lib.spq_linear_lora_fwd(ctypes.byref(args), pkg._lib.stream_ptr(DEV))
    pkg._lib.check(rc, "spq_linear_lora_fwd(levels out)")
    torch.cuda.synchronize()
    yn = y.cpu().numpy()
    if epilogue == pkg._lib.EPILOGUE_NONE:                         # the construction itself: y walks bias's float neighbours
        np.testing.assert_array_equal(yn, (x + bias[None]).astype(np.float32))
    return yn


def _pow2(e):
    return np.array([2.0 ** e, 2.0 ** -e], np.float32)


# bits, qtype, sym, epilogue (0 NONE, 1 GELU)
LV2_CASES = [(3, "log", True, 0), (4, "log", False, 0), (8, "log", True, 0), (12, "log", False, 0), (16, "log", True, 0),
             (6, "log_direct", True, 0), (18, "log_direct", False, 0), (10, "log_direct", True, 0),
             (8, "log", True, 1), (13, "log", False, 1)]


@pytest.mark.parametrize("bits,qtype,sym,epi", LV2_CASES, ids=lambda v: str(v))
def test_levels_out_limbs_at_ties(pkg, bits, qtype, sym, epi):
    """LV = 2: two fp16 limbs of FQ(y) * 2^G for a log consumer, decided on the very y the kernel stored.  Under GELU the ties
    are placed above 2^3, where gelu is the identity in fp32, and the exact chain runs on the stored (post-GELU) y."""
    direct = qtype == "log_direct"
    N, Q = 512, 127
    bias, s, mins, ranges = L.bias_ties(bits, sym, N, min_lg=3.0 if epi else None, max_lg=20.0, signed=not epi, seed=bits + 50 * epi)
    q0 = L.levels(L.walk(bias, s, Q), mins[None], ranges[None], bits, sym)
    bound = np.abs(L.dequant(L.walk(bias, s, Q), q0, mins[None], ranges[None], bits, sym, direct)).max()
    G = 13 - int(np.ceil(np.log2(bound)))
    hi = torch.zeros(256, N, dtype=torch.float16, device=DEV)
    lo = torch.zeros(256, N, dtype=torch.float16, device=DEV)
    code = pkg._lib.QTYPE_ANY[qtype]
    y = _store_forward(pkg, bias, s, Q, epi, (hi, lo, _t(ranges), _t(mins), code, bits, sym, _t(_pow2(G))))
    tag = f"levels-out {bits}-bit {qtype} sym={sym} epilogue={epi}"
    q, o, amb = _case(y, mins[None], ranges[None], bits, sym, direct, tag)
    tol = L.limb_tol(o, 2.0 ** -G)
    sep = L.separable(y, q, o, mins[None], ranges[None], bits, sym, direct, tol=tol)
    _coverage(y, mins[None], ranges[None], bits, sym, sep, tag)
    got = L.limb_decode(hi.cpu().numpy(), lo.cpu().numpy(), 2.0 ** -G)
    _assert_within(got, o, tol, amb, tag)


@pytest.mark.parametrize("bits", [4, 8, 12])
def test_levels_out_minmax_at_ties(pkg, bits):
    """LV = 1: q = clamp(rint(y / s[n]), +-qhi) with y on (k + 1/2) s[n] and its neighbours: torch.round(y / s) bit for bit."""
    N, Q = 256, 40
    qhi = (1 << (bits - 1)) - 1
    rng = np.random.default_rng(bits)
    so = np.exp2(rng.integers(-8, 4, N)).astype(np.float32)
    k = rng.integers(-qhi - 1, qhi + 1, N).astype(np.float32)
    bias = ((k + np.float32(0.5)) * so).astype(np.float32)
    s = L.ulp_pow2(bias)
    hi = torch.full((256, N), 1000.0, dtype=torch.float16, device=DEV)
    y = _store_forward(pkg, bias, s, Q, 0, (hi, None, _t(so), None, pkg._lib.MINMAX, bits, True, None))
    ref = torch.round(torch.from_numpy(y) / torch.from_numpy(so)[None]).clamp(-qhi, qhi)
    ties = int((np.abs(y / so - np.rint(y / so)) == 0.5).sum())
    print(f"levels-out min-max {bits}-bit: {ties} on k+1/2")
    assert ties >= MIN_EXACT
    assert torch.equal(hi.cpu().float(), ref)
