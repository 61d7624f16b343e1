"""GPU: the causal attention core ``spq_causal_attention_fwd`` (csrc/spq_attention.hip) through the C ABI -- parity
against the float64 oracle, the log-sum-exp output, determinism, batch / prefix invariance, NaN rows, stream capture -- and
``SPAttention.use_hip_core`` inside a block and a model (values, launch trace, the gradient path).

The bar.  ``oracle.ref_cpu.attention_core`` in float64 on the CPU is the yardstick.  The fp32 oracle itself is not far inside
the project's bar 1e-5 |y| + 1e-5 rms(y) on this operation (err/bound 0.30 on randn, 0.7 .. 0.8 on the wider standard cases below,
1.6 on randn x 3), so each case is judged like the LayerNorm gradients: the test measures e_ref, the fp32 oracle's err/bound
against float64, and the kernel must be within the bar times (1 + e_ref), no element excluded.  The standard cases assert
e_ref <= 1; randn x 3 is a declared stress case with its own e_ref."""
import math
import types

import pytest
import torch

from helpers import rows_outside
from test_blocks_cpu import load_blk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNEL = "causal_attention_fwd_kernel"


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    return p


def cabi(pkg, qkv, n_head, want_lse=False):
    """spq_causal_attention_fwd on a [B, T, 3C] device tensor -> (out [B, T, C], lse [B, H, T] or None)"""
    B, T, C3 = qkv.shape
    C = C3 // 3
    out = torch.full((B, T, C), float("nan"), device=qkv.device)
    lse = torch.full((B, n_head, T), float("nan"), device=qkv.device) if want_lse else None
    L = pkg._lib
    rc = L.load().spq_causal_attention_fwd(qkv.data_ptr(), B, T, n_head, C // n_head, out.data_ptr(), L.ptr(lse), L.stream_ptr(qkv.device))
    L.check(rc, "spq_causal_attention_fwd")
    return out, lse


def oracle(qkv_cpu, n_head, dtype, chunk=4):
    """oracle.ref_cpu.attention_core in ``dtype``, a few sequences at a time (they are independent)"""
    from oracle import ref_cpu as O
    return torch.cat([O.attention_core(qkv_cpu[i:i + chunk].to(dtype), n_head) for i in range(0, qkv_cpu.shape[0], chunk)])


def lse_ref(qkv_cpu, n_head, dtype, chunk=4):
    """logsumexp over j <= t of q_t . k_j / sqrt(d), [B, H, T]"""
    outs = []
    for i in range(0, qkv_cpu.shape[0], chunk):
        x = qkv_cpu[i:i + chunk].to(dtype)
        B, T, C3 = x.shape
        C = C3 // 3
        d = C // n_head
        q, k, _ = x.split(C, dim=2)
        q = q.view(B, T, n_head, d).transpose(1, 2)
        k = k.view(B, T, n_head, d).transpose(1, 2)
        att = (q @ k.transpose(-2, -1)) / math.sqrt(d)
        att = att.masked_fill(torch.tril(torch.ones(T, T)) == 0, float("-inf"))
        outs.append(torch.logsumexp(att, dim=-1))
    return torch.cat(outs)


def judge(got, ref32, ref64, what, standard=True):
    """err/bound of ``got`` and of the fp32 reference against float64 under 1e-5 |y| + 1e-5 rms(y); asserts the widened bar."""
    y = ref64.double()
    bound = 1e-5 * y.abs() + 1e-5 * float(y.pow(2).mean().sqrt())
    e_ref = float(((ref32.double() - y).abs() / bound).max())
    e = float(((got.detach().cpu().double() - y).abs() / bound).max())
    print(f"[attention] {what}: kernel err/bound {e:.3f}, fp32 oracle err/bound {e_ref:.3f}, allowed {1 + e_ref:.3f}")
    if standard:
        assert e_ref <= 1.0, f"{what}: not a standard case, the fp32 oracle itself is at {e_ref:.3f}"
    assert e <= 1.0 + e_ref, f"{what}: err/bound {e:.3f} > 1 + e_ref = {1 + e_ref:.3f}"
    return e, e_ref


def make_qkv(B, T, H, d, scale=1.0, offset=0.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, 3 * H * d, generator=g) * scale + offset


def check_case(pkg, qkv, H, what, standard=True, with_lse=True):
    out, lse = cabi(pkg, qkv.to(DEV), H, want_lse=with_lse)
    res = judge(out, oracle(qkv, H, torch.float32), oracle(qkv, H, torch.float64), what, standard)
    if with_lse:
        judge(lse, lse_ref(qkv, H, torch.float32), lse_ref(qkv, H, torch.float64), what + " (lse)", standard=False)
    return res


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
STANDARD = {                      # (B, T, heads, head_dim, scale, offset)
    "x1": (2, 1024, 12, 64, 1.0, 0.0),
    "offset2": (2, 1024, 12, 64, 1.0, 2.0),
    "x2_T1000": (2, 1000, 12, 64, 2.0, 0.0),
    "x1.5_16x80": (2, 1024, 16, 80, 1.5, 0.0),
    "B3_T77_4x32": (3, 77, 4, 32, 1.0, 0.0),
}


@pytest.mark.parametrize("name", list(STANDARD))
def test_parity_standard_cases(pkg, name):
    B, T, H, d, scale, offset = STANDARD[name]
    check_case(pkg, make_qkv(B, T, H, d, scale, offset, seed=11), H, name, standard=True)


def test_parity_stress_x3(pkg):
    """randn x 3: the fp32 oracle itself leaves the plain bar here (e_ref about 1.6); judged at 1 + its own e_ref"""
    check_case(pkg, make_qkv(2, 1024, 12, 64, 3.0, 0.0, seed=11), 12, "x3 (stress)", standard=False)


@pytest.mark.parametrize("B,T,H,d", [(1, 1, 12, 64), (2, 63, 12, 64), (2, 64, 16, 64), (1, 65, 12, 64), (1, 1000, 16, 64),
                                     (32, 129, 12, 64), (1, 1024, 16, 64), (2, 300, 3, 128), (2, 200, 5, 16)])
def test_parity_shapes(pkg, B, T, H, d):
    check_case(pkg, make_qkv(B, T, H, d, seed=B * 1000 + T), H, f"B{B} T{T} {H}x{d}", standard=True)


def test_parity_config3_size(pkg):
    """the full config-3 core: 32 sequences x 12 heads x 1024 x 64"""
    check_case(pkg, make_qkv(32, 1024, 12, 64, seed=3), 12, "config 3 (32 x 12 x 1024 x 64)", standard=True)


def _fixture_block(pkg, name="block_mm4"):
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
    pkg.calibrate_model(blk, bits, [t["x0"].to(DEV), t["x1"].to(DEV)])
    return blk, t, meta


def test_parity_on_the_fixture_blocks_own_qkv(pkg):
    """real data: c_attn of the reference-shaped fixture block on its input, the core on the product's own qkv"""
    blk, t, meta = _fixture_block(pkg)
    with torch.no_grad():
        qkv = blk.attn.c_attn(blk.ln_1(t["x2"].to(DEV))).contiguous()
    out, _ = cabi(pkg, qkv, meta["H"])
    q = qkv.cpu()
    judge(out, oracle(q, meta["H"], torch.float32), oracle(q, meta["H"], torch.float64), "fixture block_mm4 qkv", standard=True)


# ---- 2. lse, determinism, invariance -------------------------------------------------------------------------------------------
def test_out_does_not_depend_on_lse_and_runs_repeat(pkg):
    qkv = make_qkv(3, 333, 12, 64, seed=21).to(DEV)
    a, lse = cabi(pkg, qkv, 12, want_lse=True)
    b, none = cabi(pkg, qkv, 12, want_lse=False)
    c, lse2 = cabi(pkg, qkv, 12, want_lse=True)
    assert none is None and torch.equal(a, b) and torch.equal(a, c) and torch.equal(lse, lse2)
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(lse).all())      # (every element was written)


def test_batch_invariance(pkg):
    qkv = make_qkv(8, 700, 12, 64, seed=22).to(DEV)
    full, lse = cabi(pkg, qkv, 12, want_lse=True)
    for part in (slice(0, 4), slice(4, 8)):
        o, s = cabi(pkg, qkv[part].contiguous(), 12, want_lse=True)
        assert torch.equal(o, full[part]) and torch.equal(s, lse[part])
    perm = torch.tensor([5, 2, 7, 0, 3, 6, 1, 4], device=DEV)
    o, s = cabi(pkg, qkv[perm].contiguous(), 12, want_lse=True)
    assert torch.equal(o, full[perm]) and torch.equal(s, lse[perm])


@pytest.mark.parametrize("Tp", [1, 64, 100, 513])
def test_prefix_invariance(pkg, Tp):
    qkv = make_qkv(2, 1024, 12, 64, seed=23).to(DEV)
    full, lse = cabi(pkg, qkv, 12, want_lse=True)
    o, s = cabi(pkg, qkv[:, :Tp].contiguous(), 12, want_lse=True)
    assert torch.equal(o, full[:, :Tp]) and torch.equal(s, lse[:, :, :Tp])


def explicit_gpu(qkv, n_head):
    """models_sp.py:61-75 on the device's stock ops"""
    B, T, C3 = qkv.shape
    C = C3 // 3
    d = C // n_head
    q, k, v = qkv.split(C, dim=2)
    q = q.view(B, T, n_head, d).transpose(1, 2)
    k = k.view(B, T, n_head, d).transpose(1, 2)
    v = v.view(B, T, n_head, d).transpose(1, 2)
    att = (q @ k.transpose(-2, -1)) / (d ** 0.5)
    att = att.masked_fill(torch.tril(torch.ones(T, T, device=qkv.device)) == 0, float("-inf"))
    return (torch.softmax(att, dim=-1) @ v).transpose(1, 2).contiguous().view(B, T, C)


def test_nan_rows(pkg):
    """One NaN in q (row 70 of head 2, sequence 0), one in k (row 200 of head 5, sequence 1), one in v (row 0 of head 7,
    sequence 0): the NaN rows are the explicit formula's, every other row keeps the bits of the clean run."""
    B, T, H, d = 2, 300, 12, 64
    C = H * d
    clean = make_qkv(B, T, H, d, seed=24).to(DEV)
    dirty = clean.clone()
    dirty[0, 70, 2 * d + 5] = float("nan")
    dirty[1, 200, C + 5 * d + 9] = float("nan")
    dirty[0, 0, 2 * C + 7 * d + 1] = float("nan")
    o_clean, _ = cabi(pkg, clean, H)
    o, lse = cabi(pkg, dirty, H, want_lse=True)
    nan_rows = torch.isnan(o).view(B, T, H, d).any(-1)
    want = torch.isnan(explicit_gpu(dirty, H)).view(B, T, H, d).any(-1)
    assert torch.equal(nan_rows, want)
    expect = torch.zeros(B, T, H, dtype=torch.bool, device=DEV)
    expect[0, 70, 2] = True
    expect[1, 200:, 5] = True
    expect[0, :, 7] = True
    assert torch.equal(nan_rows, expect)
    keep = ~nan_rows.unsqueeze(-1).expand(B, T, H, d).reshape(B, T, C)
    assert torch.equal(o[keep], o_clean[keep])
    assert bool(torch.isnan(lse[0, 2, 70])) and bool(torch.isnan(lse[1, 5, 200:]).all()) and not bool(torch.isnan(lse[0, 7]).any())


def test_nan_in_v_stays_causal(pkg):
    """A NaN in v-row j reaches rows >= j and nothing before j's own 32-key tile (here j = 96 starts one, so: nothing before j).
    The dense formula's 0 * NaN spreads it to every row of the head; the kernel never multiplies the tiles above the diagonal."""
    B, T, H, d = 1, 200, 4, 64
    clean = make_qkv(B, T, H, d, seed=25).to(DEV)
    dirty = clean.clone()
    dirty[0, 96, 2 * H * d + 3 * d + 17] = float("nan")
    o_clean, _ = cabi(pkg, clean, H)
    o, _ = cabi(pkg, dirty, H)
    nan_rows = torch.isnan(o).view(B, T, H, d).any(-1)
    expect = torch.zeros(B, T, H, dtype=torch.bool, device=DEV)
    expect[0, 96:, 3] = True
    assert torch.equal(nan_rows, expect)
    assert torch.equal(torch.isnan(o).view(B, T, H, d)[0, 96:, 3].sum(0).nonzero().flatten().cpu(), torch.tensor([17]))
    keep = ~torch.isnan(o)
    assert torch.equal(o[keep], o_clean[keep])


# ---- 3. the Python surface and the modules -------------------------------------------------------------------------------------
def _launched(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_python_entry_point(pkg):
    qkv = make_qkv(2, 130, 12, 64, seed=26).to(DEV)
    want, want_lse = cabi(pkg, qkv, 12, want_lse=True)
    out, lse = pkg.causal_attention(qkv, 12, return_lse=True)
    assert torch.equal(out, want) and torch.equal(lse, want_lse)
    assert torch.equal(pkg.causal_attention(qkv, 12), want)
    with pytest.raises(RuntimeError):
        pkg.causal_attention(qkv.cpu(), 12)
    with pytest.raises(TypeError):
        pkg.causal_attention(qkv.half(), 12)
    with pytest.raises(pkg._lib.SpqError):
        pkg.causal_attention(make_qkv(1, 8, 2, 48).to(DEV), 2)              # head_dim 48: no kernel, and no fall-back here
    with pytest.raises(ValueError):
        pkg.causal_attention(qkv[:, :, :-3], 12)


def _block(pkg, bits=4, r=16, E=768, H=12, T=1024):
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


def _sdpa_only_kernels(B, T, H, d, explicit_names):
    """names of the kernels a bare scaled_dot_product_attention launches on head-split views that the explicit run does not"""
    qkv = torch.randn(B, T, 3 * H * d, device=DEV)
    q, k, v = (p.view(B, T, H, d).transpose(1, 2) for p in qkv.split(H * d, dim=2))
    names = _launched(lambda: torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True))
    only = set(names) - set(explicit_names)
    assert only, names
    return only


def _cores_of(module, x, pkg, forward=None):
    """{core: (final output, [core inputs], [core outputs], kernel names)} of an eval forward under each attention core"""
    res = {}
    attns = [m for m in module.modules() if isinstance(m, pkg.SPAttention)]
    for core in ("explicit", "sdpa", "hip"):
        assert pkg.set_attention_core(module, core) == len(attns)
        ins, outs, hooks = [], [], []
        for a in attns:
            orig = a.core

            def wrapped(qkv, _orig=orig):
                ins.append(qkv)
                outs.append(_orig(qkv))
                return outs[-1]
            a.core = wrapped
            hooks.append(a)
        try:
            with torch.no_grad():
                y = module(x)
                for a in hooks:
                    del a.core
                names = _launched(lambda: module(x))
                assert torch.equal(module(x), y)
        finally:
            for a in hooks:
                a.__dict__.pop("core", None)
        res[core] = (y, ins, outs, names)
    pkg.set_attention_core(module, "sdpa")
    return res


def _check_module(pkg, module, x, H, d, what):
    res = _cores_of(module, x, pkg)
    names_hip, names_exp = res["hip"][3], res["explicit"][3]
    B, T = x.shape[0], x.shape[1]
    sdpa_only = _sdpa_only_kernels(B, T, H, d, names_exp)
    n_attn = len(res["hip"][1])
    assert sum(KERNEL in n for n in names_hip) >= n_attn, names_hip                 # the library's kernel ran, once per attention
    assert not (sdpa_only & set(names_hip)), sdpa_only & set(names_hip)             # ... and no SDPA kernel did: no quiet fall-back
    assert sdpa_only <= set(res["sdpa"][3]) and not any(KERNEL in n for n in res["sdpa"][3] + names_exp)
    # the first core sees bit-identical qkv under every setting: judge it against float64 on that qkv
    qkv = res["hip"][1][0]
    assert torch.equal(qkv, res["explicit"][1][0])
    q = qkv.cpu()
    judge(res["hip"][2][0], oracle(q, H, torch.float32), oracle(q, H, torch.float64), what + ": first core output", standard=False)
    # chained-test condition: a last-ulp change at the core can move a level of c_proj's input
    y_exp = res["explicit"][0]
    for core in ("sdpa", "hip"):
        off = rows_outside(res[core][0].reshape(-1, y_exp.shape[-1]), y_exp.reshape(-1, y_exp.shape[-1]), 1e-5)
        frac = float(off.float().mean())
        print(f"[attention] {what}: {core} vs explicit, rows outside 1e-5: {frac:.4%}")
        assert frac <= 0.02, (what, core, frac)


def test_block_on_the_hip_core(pkg):
    bits = 4
    blk = _block(pkg, bits)
    g = torch.Generator().manual_seed(1)
    x0, x1, x2 = (torch.randn(2, 1024, 768, generator=g).to(DEV) for _ in range(3))
    pkg.calibrate_model(blk, bits, [x0, x1])
    _check_module(pkg, blk, x2, 12, 64, "SPBlock 2 x 1024 x 768, 4-bit")


def test_model_on_the_hip_core(pkg):
    bits, E, H, T = 4, 256, 4, 128
    cfg = types.SimpleNamespace(vocab_size=1000, n_positions=T, n_embd=E, n_layer=3, n_head=H, layer_norm_epsilon=1e-5,
                                embd_pdrop=0.0, bit_widths=[bits, 32], lora_rank_per_bit={bits: 16, 32: 0},
                                lora_alpha_per_bit={bits: 32, 32: 0}, quantizer_per_bit={bits: "minmax", 32: None},
                                per_channel_quantization=True)
    torch.manual_seed(0)
    model = pkg.SPModel(cfg)
    with torch.no_grad():
        for n, p_ in model.named_parameters():
            if "lora_B" in n:
                p_.normal_(0, 0.01)
            elif p_.dim() > 1 and "lora_A" not in n:
                p_.normal_(0, 0.02)
    model = model.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    mk = lambda n: torch.randint(0, cfg.vocab_size, (n, T), generator=g).to(DEV)
    pkg.calibrate_model(model, bits, [mk(4) for _ in range(2)])
    _check_module(pkg, model, mk(4), H, E // H, "SPModel 3 layers, 4 x 128 x 256, 4-bit")


def test_gradient_takes_the_old_path(pkg):
    """flag on + a gradient required: SDPA runs (the kernel has no backward), and the gradients are the flag-off run's, bit for bit"""
    bits = 4
    blk = _block(pkg, bits, E=256, H=4, T=256)
    g = torch.Generator().manual_seed(2)
    x0, x1, x2 = (torch.randn(2, 256, 256, generator=g).to(DEV) for _ in range(3))
    pkg.calibrate_model(blk, bits, [x0, x1])
    blk.train()
    for lin in (blk.attn.c_attn, blk.attn.c_proj, blk.mlp.c_fc, blk.mlp.c_proj):     # base weights frozen (main_sp.py:83)
        lin.linear.weight.requires_grad_(False)
        lin.linear.bias.requires_grad_(False)

    def grads(core):
        pkg.set_attention_core(blk, core)
        blk.zero_grad(set_to_none=True)
        x = x2.clone().requires_grad_(True)
        names = _launched(lambda: blk(x).square().sum().backward())
        return names, [x.grad] + [p.grad for p in blk.parameters() if p.grad is not None]
    grads("sdpa")                                      # untimed first step: one-time launches (operand caches) stay out of the traces
    names_off, g_off = grads("sdpa")
    names_on, g_on = grads("hip")
    names_exp, _ = grads("explicit")
    sdpa_only = set(names_off) - set(names_exp)        # what SDPA's forward and backward launch and the explicit formula does not
    print(f"[attention] gradient path: SDPA-only kernels {sorted(sdpa_only)}; on ^ off {sorted(set(names_on) ^ set(names_off))}")
    assert sdpa_only, names_off
    assert not any(KERNEL in n for n in names_on + names_off + names_exp)
    assert sdpa_only <= set(names_on), sdpa_only - set(names_on)
    assert len(g_on) == len(g_off) > 1
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b)
    pkg.set_attention_core(blk, "hip")
    with torch.no_grad():                                                       # the same module without a gradient: the kernel
        assert any(KERNEL in n for n in _launched(lambda: blk(x2)))
    pkg.set_attention_core(blk, "sdpa")


def test_stream_capture_replays(pkg):
    qkv = make_qkv(2, 257, 12, 64, seed=27).to(DEV)
    want, want_lse = pkg.causal_attention(qkv, 12, return_lse=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lse = pkg.causal_attention(qkv, 12, return_lse=True)
    for _ in range(2):
        out.fill_(float("nan"))
        lse.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(lse, want_lse)
    qkv.copy_(make_qkv(2, 257, 12, 64, seed=28))                               # new contents, same addresses
    graph.replay()
    torch.cuda.synchronize()
    fresh, fresh_lse = pkg.causal_attention(qkv, 12, return_lse=True)
    assert torch.equal(out, fresh) and torch.equal(lse, fresh_lse)
