"""GPU parity of the FP6 operand path (SPQ_PATH_FP6: e2m3 activation levels x five radix-32 digit planes of the integer weight on
v_mfma_scale_f32_16x16x128_f8f6f4; csrc/spq_fp6_kernel.h) against the reference's fixtures and the CPU oracle, at the project's own
bar |d| <= 1e-5 |y_ref| + 1e-5 rms(y_ref).  Every case asserts the path the forward took, so a silent fall-back fails."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import fp6_ref as F6
from helpers import GOLDEN, assert_close_y, load_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    return p


def build_layer(pkg, meta, t, path):
    bits, r = meta["bits"], meta["r"]
    layer = pkg.SPLinearWithLoRA(meta["K"], meta["N"], [bits, 32], {bits: r, 32: 0}, {bits: meta["alpha"], 32: 0},
                                 {bits: meta["qtype"], 32: None}, per_channel=meta["per_channel"])
    key = f"{bits}bit"
    with torch.no_grad():
        layer.linear.weight.copy_(t["W"]); layer.linear.bias.copy_(t["bias"])
        layer.lora_adapters[key].lora_A.copy_(t["A"]); layer.lora_adapters[key].lora_B.copy_(t["B"])
    layer = layer.to(DEV).eval()
    layer.set_precision(bits)
    layer.operand_path = path
    pkg.calibrate_layer(layer, bits, [t["x0"].to(DEV), t["x1"].to(DEV)])
    return layer, key


def make_pair_from(pkg, W, bias, A, B, x0, x1, bits, qtype, per_channel, alpha=None, path=None):
    """(product layer on GPU, calibrated oracle layer): the recipe of test_gpu_shapes.make_pair"""
    from oracle import ref_cpu as O
    N, K = W.shape
    r = A.shape[1]
    alpha = r if alpha is None else alpha
    ol = O.build_calibrated_layer(W, bias, A, B, [x0, x1], bits, qtype, per_channel, alpha, r, symmetric=True)
    layer = pkg.SPLinearWithLoRA(K, N, [bits, 32], {bits: r, 32: 0}, {bits: alpha, 32: 0}, {bits: qtype, 32: None}, per_channel=per_channel)
    key = f"{bits}bit"
    with torch.no_grad():
        layer.linear.weight.copy_(W); layer.linear.bias.copy_(bias)
        layer.lora_adapters[key].lora_A.copy_(A); layer.lora_adapters[key].lora_B.copy_(B)
    layer = layer.to(DEV).eval()
    layer.set_precision(bits)
    layer.operand_path = pkg._lib.PATH_FP6 if path is None else path
    pkg.calibrate_layer(layer, bits, [x0.to(DEV), x1.to(DEV)])
    return layer, ol


def make_pair(pkg, M, K, N, r, bits, qtype, per_channel, seed, batch=4, path=None):
    from oracle import ref_cpu as O
    W, bias, A, B, x0, x1 = O.make_workload(M, K, N, r, seed=seed, batch=batch)
    layer, ol = make_pair_from(pkg, W, bias, A, B, x0, x1, bits, qtype, per_channel, path=path)
    return layer, ol, x0, x1


# ---- 1. fixtures
@pytest.mark.parametrize("name", ["mm3_pc", "mm4_pc", "mm4_pc_edge", "mm4_pc_ragged", "mm4_pt_zeroB"])
def test_fixture_on_fp6(pkg, name):
    meta, t = load_case(name)
    L = pkg._lib
    layer, key = build_layer(pkg, meta, t, L.PATH_FP6)
    lora = layer.lora_adapters[key]
    quants = {"qx": layer.quantizers_input[key], "qw": layer.quantizers_weight[key], "qA": lora.quantize_A, "qB": lora.quantize_B}
    with torch.no_grad():
        for tag, q in quants.items():
            if tuple(q.scale.shape) == tuple(t[f"{tag}.scale"].shape):
                q.scale = t[f"{tag}.scale"].to(DEV); q.zero_point = t[f"{tag}.zero_point"].to(DEV); q._epoch += 1
        y2 = layer(t["x2"].to(DEV))
        assert layer._last_path == L.PATH_FP6, layer._last_path
        y0 = layer(t["x0"].to(DEV))
        y2d = layer(t["x2"].reshape(-1, meta["K"])[:40].contiguous().to(DEV))
        assert layer._last_path == L.PATH_FP6
        layer.calibration_mode = True
        base = layer(t["x2"].to(DEV))
        assert layer._last_path == L.PATH_F16X2, layer._last_path           # no LoRA term: the fp16 levels carry a NaN, e2m3 cannot
        layer.calibration_mode = False
        layer.cache_operands = False                                          # the re-quantising forward: one C call with `prepare` set
        for fuse in (False, True):
            layer.fuse_prepare = fuse
            assert torch.equal(layer(t["x2"].to(DEV)), y2)
            assert layer._last_path == L.PATH_FP6
    assert torch.isfinite(y2).all()
    assert_close_y(y2, t["y_x2"], f"{name}.y_x2[fp6]", 1e-5)
    assert_close_y(y0, t["y_x0"], f"{name}.y_x0[fp6]", 1e-5)
    assert_close_y(y2d, t["y_2d"], f"{name}.y_2d[fp6]", 1e-5)
    assert_close_y(base, t["base_x2"], f"{name}.base_x2", 1e-5)


# ---- 2. shapes
SHAPES = [
    ("c_attn_4bit",     2048, 768,  2304, 64,  4, True),
    ("attn_cproj_4bit", 2048, 768,  768,  64,  4, True),
    ("mlp_cproj_4bit",  2048, 3072, 768,  64,  4, True),
    ("ragged_rank16",   1000, 320,  200,  16,  4, True),
    ("tiny",            3,    64,   8,    8,   3, False),
    ("rank128",         512,  256,  384,  128, 4, True),
    ("rank100_K72",     300,  72,   260,  100, 4, True),
    ("bits2",           512,  256,  256,  32,  2, True),
    ("ragged_N_101",    300,  128,  101,  16,  4, True),
    ("headline_cfc",    8192, 768,  3072, 64,  4, True),
]


@pytest.mark.parametrize("name,M,K,N,r,bits,pc", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes_against_oracle(pkg, name, M, K, N, r, bits, pc):
    batch = 4 if M % 4 == 0 else 1
    layer, ol, x0, x1 = make_pair(pkg, M, K, N, r, bits, "minmax", pc, seed=zlib.crc32(name.encode()) % 1000, batch=batch)
    with torch.no_grad():
        y = layer(x0.to(DEV))
        assert layer._last_path == pkg._lib.PATH_FP6
        y_again = layer(x0.to(DEV))
    assert torch.equal(y, y_again)                                            # 5. determinism
    assert_close_y(y, ol.forward(x0), name, 1e-5)


# ---- 3. operands against the oracle
def _weight_prime(ol, K):
    """W'[n,k] = FQ(W)[n,k] * sx[k] in float64 (the exact product) from the oracle's quantizers"""
    fqw = ol.qw(ol.W).double().numpy()
    sx = ol.qx.scale.double().reshape(-1).numpy()
    return fqw * (sx[None, :] if sx.size > 1 else sx[0])


def _check_operands(pkg, layer, ol, x, key):
    L = pkg._lib
    M = x.reshape(-1, x.shape[-1]).shape[0]
    N, K = ol.W.shape
    with torch.no_grad():
        y = layer(x.to(DEV))
    assert layer._last_path == L.PATH_FP6
    torch.cuda.synchronize()
    # activation levels: the packed plane at byte 0 of the forward's workspace (include/spq.h, SPQ_PATH_FP6)
    ws = L.workspace(DEV, 1, L.stream_ptr(DEV))
    nb = F6.plane_bytes(M, K, 256)
    plane = ws[:nb].cpu().numpy()
    got = F6.e2m3_decode(F6.unpack(plane, M, K, 256))
    assert not F6.unpack_full(plane, M, K, 256)[:M, K:].any(), "the k padding of the activation plane must hold the zero code"
    want = ol.qx.levels(x.reshape(-1, K)).double().numpy().reshape(M, K)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} activation levels differ from the oracle's"
    # weight digits: five planes at byte 0 of w_prep, row scales in w_rowscale
    prep = layer._prepared[(key, L.PATH_FP6)]
    pb = F6.plane_bytes(N, K, 128)
    planes = prep.w[:5 * pb].cpu().numpy().reshape(5, pb)
    w = F6.unpack_weight(planes, N, K)
    wp = _weight_prime(ol, K)
    rs = prep.w_rowscale[:N].cpu().double().numpy()
    E = np.rint(-np.log2(rs)).astype(np.int64)
    assert np.array_equal(np.exp2(-E.astype(np.float64)), rs), "rowscale is not a power of two"
    mx = np.abs(wp).max(axis=1)
    live = mx > 0
    scaled = mx * np.exp2(E.astype(np.float64))
    assert np.all((scaled[live] >= 2.0 ** 23) & (scaled[live] < 2.0 ** 24)), "row exponent rule"
    assert np.array_equal(E[live], F6.row_exponent(wp)[live])
    want_w = np.rint(np.ldexp(wp, E[:, None])).astype(np.int64)
    assert np.array_equal(w, want_w), f"{int((w != want_w).sum())} of {w.size} weight integers differ from rint(W' 2^E) in float64"
    full = np.stack([F6.unpack_full(planes[i], N, K, 128) for i in range(5)])
    assert not full[:, N:].any() and not full[:, :, K:].any(), "padding rows / columns must hold the zero code"
    return y


@pytest.mark.parametrize("name,M,K,N,r,bits,pc", [s for s in SHAPES if s[0] in ("ragged_rank16", "rank100_K72", "tiny", "attn_cproj_4bit", "bits2")],
                         ids=lambda v: v if isinstance(v, str) else None)
def test_operands_against_oracle(pkg, name, M, K, N, r, bits, pc):
    layer, ol, x0, _ = make_pair(pkg, M, K, N, r, bits, "minmax", pc, seed=zlib.crc32(name.encode()) % 1000 + 1, batch=4 if M % 4 == 0 else 1)
    _check_operands(pkg, layer, ol, x0, f"{bits}bit")


def test_zero_rows_give_finite_output(pkg):
    from oracle import ref_cpu as O
    W, bias, A, B, x0, x1 = O.make_workload(320, 192, 160, 16, seed=5, batch=4)
    W = W.clone(); W[7] = 0.0; W[128:160] = 0.0
    B = B.clone(); B[:, 3] = 0.0
    layer, ol = make_pair_from(pkg, W, bias, A, B, x0, x1, 4, "minmax", True)
    y = _check_operands(pkg, layer, ol, x0, "4bit")
    assert torch.isfinite(y).all()
    assert_close_y(y, ol.forward(x0), "zero rows", 1e-5)
    meta, t = load_case("mm4_pt_zeroB")
    layer, key = build_layer(pkg, meta, t, pkg._lib.PATH_FP6)
    with torch.no_grad():
        y = layer(t["x2"].to(DEV))
    assert layer._last_path == pkg._lib.PATH_FP6 and torch.isfinite(y).all()


# ---- 4. epilogue / prologue
def test_gelu_store(pkg):
    layer, ol, x0, _ = make_pair(pkg, 1024, 256, 512, 32, 4, "minmax", True, seed=11)
    with torch.no_grad():
        y = layer(x0.to(DEV), activation="gelu")
    assert layer._last_path == pkg._lib.PATH_FP6 and layer._activation_fused
    assert_close_y(y, torch.nn.functional.gelu(ol.forward(x0)), "gelu store", 1e-5)


def test_layernorm_prologue_bit_identical(pkg):
    from oracle import ref_cpu as O
    M, K, N, r = 1000, 768, 512, 16
    W, bias, A, B, x0, x1 = O.make_workload(M, K, N, r, seed=21, batch=1)
    L = pkg._lib
    g = torch.Generator().manual_seed(3)
    lw, lb = 1.0 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
    raw0, raw1 = 3.0 * x0 + 0.5, 2.0 * x1 - 0.25
    n0, n1 = O.switchable_layernorm(raw0, lw, lb), O.switchable_layernorm(raw1, lw, lb)
    layer, ol = make_pair_from(pkg, W, bias, A, B, n0, n1, 4, "minmax", True)
    lib = L.load()
    xin = raw0.to(DEV).contiguous()
    normed = torch.empty_like(xin)
    lwd, lbd = lw.to(DEV), lb.to(DEV)
    L.check(lib.spq_layernorm(xin.data_ptr(), M, K, lwd.data_ptr(), lbd.data_ptr(), 1e-5, normed.data_ptr(), L.stream_ptr(DEV)), "spq_layernorm")
    with torch.no_grad():
        y_plain = layer(normed)
    assert layer._last_path == L.PATH_FP6
    assert_close_y(y_plain, ol.forward(normed.cpu()), "layer on spq_layernorm's output", 1e-5)
    # the fused prologue through the C ABI: same arguments plus ln_weight / ln_bias, x = the LayerNorm's input
    key = "4bit"
    prep = layer._prepared[(key, L.PATH_FP6)]
    qx = layer.quantizers_input[key]
    sx, zx = qx.qparams_for(K)
    y = torch.empty(M, N, dtype=torch.float32, device=DEV)
    ws = torch.full((lib.spq_fwd_workspace_bytes(M, K, N, r, L.PATH_FP6),), 0xFF, dtype=torch.uint8, device=DEV)
    a = L.FwdArgs(M=M, K=K, N=N, r=r, bits=4, qtype=0, symmetric=1, quantize_input=1, x_per_channel=1 if sx.numel() > 1 else 0, path=L.PATH_FP6,
                  x=xin.data_ptr(), sx=sx.data_ptr(), zx=zx.data_ptr(), w_prep=prep.w.data_ptr(), w_rowscale=prep.w_rowscale.data_ptr(),
                  bias=layer.linear.bias.data_ptr(), a_prep=prep.a.data_ptr(), b_prep=prep.b.data_ptr(),
                  lora_scaling=float(layer.lora_adapters[key].scaling), y=y.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                  ln_weight=lwd.data_ptr(), ln_bias=lbd.data_ptr(), ln_eps=1e-5)
    L.check(lib.spq_linear_lora_fwd(a, L.stream_ptr(DEV)), "spq_linear_lora_fwd(fp6 + LayerNorm)")
    torch.cuda.synchronize()
    assert torch.equal(y, y_plain.reshape(M, N)), "fused LayerNorm prologue differs from the layer run on spq_layernorm's output"


def _block(pkg, bits=4, r=16, E=768, H=12, T=1024):
    import types
    cfg = types.SimpleNamespace(n_embd=E, n_head=H, n_positions=T, layer_norm_epsilon=1e-5, bit_widths=[bits, 32],
                                lora_rank_per_bit={bits: r, 32: 0}, lora_alpha_per_bit={bits: 2 * r, 32: 0},
                                quantizer_per_bit={bits: "minmax", 32: None}, per_channel_quantization=True)
    torch.manual_seed(0)
    blk = pkg.SPBlock(cfg, bit_widths=[bits, 32])
    with torch.no_grad():
        for n, p_ in blk.named_parameters():
            if "lora_B" in n:
                p_.copy_(0.02 * torch.randn_like(p_))
    return blk.to(DEV).eval()


def test_block_on_fp6_cosim(pkg):
    """config-3 dims, 2 x 1024 tokens, every linear pinned to FP6: stage-by-stage bounds, oracle input levels, staged == fused"""
    from helpers import cosim_block
    bits = 4
    blk = _block(pkg, bits)
    g = torch.Generator().manual_seed(1)
    x0, x1, x2 = (torch.randn(2, 1024, 768, generator=g).to(DEV) for _ in range(3))
    pkg.calibrate_model(blk, bits, [x0, x1])
    lins = [blk.attn.c_attn, blk.attn.c_proj, blk.mlp.c_fc, blk.mlp.c_proj]
    for lin in lins:
        lin.operand_path = pkg._lib.PATH_FP6
    cosim_block(blk, bits, x2)
    for lin in lins:
        assert lin._last_path == pkg._lib.PATH_FP6, lin._last_path
    assert blk.mlp.c_fc._activation_fused
    with torch.no_grad():                                                     # SPMLP alone on FP6 == the block's MLP stages
        h = blk.ln_2(x2)
        m = blk.mlp(h)
        ref = blk.mlp.c_proj(blk.mlp.c_fc(h, activation="gelu"))
    assert torch.equal(m, ref)


# ---- 5. batch invariance
def test_batch_invariance(pkg):
    L = pkg._lib
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    M, K, N, r = 64 * cus + 37, 768, 768, 64
    from oracle import ref_cpu as O
    W, bias, A, B, x0, x1 = O.make_workload(M, K, N, r, seed=31, batch=1)
    layer, ol = make_pair_from(pkg, W, bias, A, B, x0, x1, 4, "minmax", True)
    xd = x0.to(DEV)

    def run(x):
        L.workspace(DEV, 1, L.stream_ptr(DEV)).fill_(0xFF)
        with torch.no_grad():
            y = layer(x.contiguous())
        assert layer._last_path == L.PATH_FP6
        return y
    full = run(xd)
    assert torch.isfinite(full).all()
    assert torch.equal(run(xd), full)
    for lo, hi in ((0, 100), (4000, 8100), (M - 77, M)):
        part = run(xd[lo:hi])
        assert torch.equal(part, full[lo:hi]), f"rows {lo}:{hi} differ from the same rows of the full batch"
    assert_close_y(full, ol.forward(x0), "batch invariance shape", 1e-5)


# ---- 6. NaN / Inf
def test_nan_and_inf_rows(pkg):
    L = pkg._lib
    layer, ol, x0, _ = make_pair(pkg, 512, 256, 384, 16, 4, "minmax", True, seed=41)
    x = x0.reshape(-1, 256).clone()
    x[17, 5] = float("nan")
    x[300, 255] = float("nan")
    with torch.no_grad():
        y = layer(x.to(DEV)).cpu().reshape(-1, 384)
    assert layer._last_path == L.PATH_FP6
    bad = torch.isnan(y).any(dim=1)
    assert bad[17] and bad[300] and int(bad.sum()) == 2 and torch.isnan(y[17]).all() and torch.isnan(y[300]).all()
    ok = ~bad
    assert_close_y(y[ok], ol.forward(x).reshape(-1, 384)[ok], "rows next to a NaN row", 1e-5)
    lora = layer.lora_adapters["4bit"]
    lora.enabled = False
    with torch.no_grad():
        y2 = layer(x.to(DEV)).cpu().reshape(-1, 384)
    assert layer._last_path == L.PATH_F16X2                                   # no LoRA term: the pinned layer falls back
    assert torch.isnan(y2[17]).all() and torch.isnan(y2[300]).all() and int(torch.isnan(y2).any(dim=1).sum()) == 2
    lora.enabled = True
    xi = x0.reshape(-1, 256).clone()
    xi[3, 9] = float("inf"); xi[200, 100] = float("-inf")
    with torch.no_grad():
        yi = layer(xi.to(DEV)).cpu().reshape(-1, 384)
    assert layer._last_path == L.PATH_FP6
    ref = ol.forward(xi).reshape(-1, 384)
    assert torch.equal(torch.isnan(yi), torch.isnan(ref)) and torch.equal(torch.isinf(yi), torch.isinf(ref))
    fin = torch.isfinite(ref).all(dim=1)
    assert torch.equal(yi[~fin].nan_to_num(nan=7.0), ref[~fin].nan_to_num(nan=7.0))
    assert_close_y(yi[fin], ref[fin], "rows next to an Inf row", 1e-5)


# ---- 7. fall-backs and the operand cache
@pytest.mark.parametrize("bits,qtype,want", [(8, "minmax", "f16x2"), (6, "log", "f16x3")])
def test_pinned_layer_falls_back(pkg, bits, qtype, want):
    L = pkg._lib
    layer, ol, x0, _ = make_pair(pkg, 512, 256, 256, 16, bits, qtype, True, seed=51)
    twin, _, _, _ = make_pair(pkg, 512, 256, 256, 16, bits, qtype, True, seed=51, path=L.PATH_AUTO)
    with torch.no_grad():
        y, yt = layer(x0.to(DEV)), twin(x0.to(DEV))
    assert L.PATH_NAMES[layer._last_path] == want and layer._last_path == twin._last_path
    assert torch.equal(y, yt)
    assert_close_y(y, ol.forward(x0), f"fall-back {qtype}{bits}", 1e-5)


def test_cache_keys_on_the_path(pkg):
    L = pkg._lib
    layer, ol, x0, _ = make_pair(pkg, 512, 256, 256, 16, 4, "minmax", True, seed=61)
    twin, _, _, _ = make_pair(pkg, 512, 256, 256, 16, 4, "minmax", True, seed=61, path=L.PATH_F16X2)
    xd = x0.to(DEV)
    with torch.no_grad():
        a = layer(xd); assert layer._last_path == L.PATH_FP6
        layer.operand_path = L.PATH_F16X2
        b = layer(xd); assert layer._last_path == L.PATH_F16X2
        layer.operand_path = L.PATH_FP6
        c = layer(xd); assert layer._last_path == L.PATH_FP6
        assert torch.equal(a, c) and torch.equal(b, twin(xd))
        layer.linear.weight.data.mul_(0.5)
        layer.invalidate_operand_cache()
        d = layer(xd); assert layer._last_path == L.PATH_FP6
    assert not torch.equal(d, a)
    from oracle import ref_cpu as O
    ol.W = ol.W * 0.5
    assert_close_y(d, ol.forward(x0), "after an in-place weight change", 1e-5)


# ---- 8. SPQ_AUTO_FP6
_CHILD = r"""
import json, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import llm_qat_on_gpt2_amd as pkg
import test_gpu_fp6 as T
from helpers import assert_close_y
L = pkg._lib
out = {}
for tag, pc in (("pc", True), ("pt", False)):
    layer, ol, x0, _ = T.make_pair(pkg, 512, 256, 256, 16, 4, "minmax", pc, seed=71, path=L.PATH_AUTO)
    with torch.no_grad():
        y = layer(x0.to(T.DEV))
    assert_close_y(y, ol.forward(x0), tag, 1e-5)
    out[tag] = layer._last_path
print("RESULT " + json.dumps(out))
"""


def test_auto_switch_in_a_child_process(pkg, tmp_path):
    L = pkg._lib
    assert os.environ.get("SPQ_AUTO_FP6") is None
    for pc, want in ((True, L.PATH_F16X2), (False, L.PATH_I8)):              # the parent: AUTO picks what it picks today
        layer, ol, x0, _ = make_pair(pkg, 512, 256, 256, 16, 4, "minmax", pc, seed=71, path=L.PATH_AUTO)
        with torch.no_grad():
            layer(x0.to(DEV))
        assert layer._last_path == want
    script = tmp_path / "auto_fp6_child.py"
    script.write_text(_CHILD)
    env = dict(os.environ, SPQ_AUTO_FP6="1")
    p = subprocess.run([sys.executable, str(script), ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res == {"pc": L.PATH_FP6, "pt": L.PATH_I8}, res


# ---- 9. gradient
def test_gradient_fixture_forward_on_fp6(pkg):
    z = np.load(os.path.join(GOLDEN, "grad_mm4_pc.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    t = {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}
    bits, r = meta["bits"], meta["r"]
    layer = pkg.SPLinearWithLoRA(meta["K"], meta["N"], [bits, 32], {bits: r, 32: 0}, {bits: meta["alpha"], 32: 0},
                                 {bits: meta["qtype"], 32: None}, per_channel=meta["per_channel"])
    key = f"{bits}bit"
    with torch.no_grad():
        layer.linear.weight.copy_(t["W"]); layer.linear.bias.copy_(t["bias"])
        layer.lora_adapters[key].lora_A.copy_(t["A"]); layer.lora_adapters[key].lora_B.copy_(t["B"])
    layer = layer.to(DEV).train()
    layer.set_precision(bits)
    layer.operand_path = pkg._lib.PATH_FP6
    pkg.calibrate_layer(layer, bits, [t["x0"].to(DEV), t["x1"].to(DEV)])
    layer.linear.weight.requires_grad_(False); layer.linear.bias.requires_grad_(False)
    xg = t["xg"].to(DEV).requires_grad_(True)
    y = layer(xg)
    assert y.grad_fn is not None and layer._last_path == pkg._lib.PATH_FP6
    assert_close_y(y, t["y"], "grad_mm4_pc.y[fp6]", 1e-5)
    y.backward(t["g"].to(DEV))
    lo = layer.lora_adapters[key]
    assert_close_y(xg.grad, t["grad_x"], "grad_x", 1e-5)
    assert_close_y(lo.lora_A.grad, t["grad_A"], "grad_A", 1e-5)
    assert_close_y(lo.lora_B.grad, t["grad_B"], "grad_B", 1e-5)


# ---- 10. fuzz inside the path's domain
@pytest.mark.parametrize("seed", list(range(100, 132)))
def test_fuzz(pkg, seed):
    rng = np.random.default_rng(seed)
    M = int(rng.integers(1, 700)); K = int(rng.integers(1, 600)); N = int(rng.integers(1, 500))
    if seed % 4 == 0:
        K = int(rng.choice([64, 128, 192, 320, 448]))                         # the streaming activation kernel
    r = int(rng.integers(1, 129)) if seed % 3 else int(rng.integers(1, 65))
    bits = int(rng.integers(2, 5)); pc = bool(rng.integers(0, 2))
    layer, ol, x0, _ = make_pair(pkg, M, K, N, r, bits, "minmax", pc, seed=seed, batch=1)
    with torch.no_grad():
        y = layer(x0.to(DEV))
    assert layer._last_path == pkg._lib.PATH_FP6
    assert_close_y(y, ol.forward(x0), f"fuzz seed {seed}: M={M} K={K} N={N} r={r} bits={bits} pc={pc}", 1e-5)


# ---- non-finite weights are not made finite
def test_non_finite_weight_row_gives_nan_column(pkg):
    """A W' row with a NaN element has no digit form: rowscale[n] is NaN and so is output column n, as the oracle's is.  An Inf
    weight is clamped to the top level by the weight quantizer, so that row stays finite, on the device as in the oracle."""
    L = pkg._lib
    layer, ol, x0, _ = make_pair(pkg, 256, 128, 96, 16, 4, "minmax", True, seed=81)
    with torch.no_grad():
        layer.linear.weight.data[5, 7] = float("nan")
        layer.linear.weight.data[40, 100] = float("inf")
        layer.invalidate_operand_cache()
        y = layer(x0.to(DEV)).cpu().reshape(-1, 96)
    assert layer._last_path == L.PATH_FP6
    ol.W = ol.W.clone(); ol.W[5, 7] = float("nan"); ol.W[40, 100] = float("inf")
    ref = ol.forward(x0).reshape(-1, 96)
    assert torch.isnan(ref[:, 5]).all() and torch.isfinite(ref[:, 40]).all()                  # what the oracle does with such weights
    assert torch.isnan(y[:, 5]).all()
    keep = [n for n in range(96) if n != 5]
    assert torch.isfinite(y[:, keep]).all()
    assert_close_y(y[:, keep], ref[:, keep], "columns next to a NaN weight row", 1e-5)
