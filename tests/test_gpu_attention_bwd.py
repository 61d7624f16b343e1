"""GPU: the causal attention backward ``spq_causal_attention_bwd`` (csrc/spq_attention_bwd.hip) through the
C ABI -- parity of dq, dk and dv against float64 CPU autograd, determinism, batch / zero-tail invariance, head independence --
then ``causal_attention_autograd`` and ``SPAttention.use_hip_backward`` inside a block (values, launch trace).

The bar (tests/attention_grad_ref.py): per third, 1e-5 |y| + 1e-5 rms(y) against float64 autograd through
``oracle.ref_cpu.attention_core``, times (1 + e_ref) with e_ref the fp32 CPU autograd's own err/bound; standard cases have
e_ref <= 1."""
import copy
import types

import pytest
import torch

from attention_grad_ref import cached_case, judge_tensor, judge_thirds, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD_KERNEL = "causal_attention_fwd_kernel"
BWD_KERNELS = ("causal_attention_bwd_delta_kernel", "causal_attention_bwd_dq_kernel", "causal_attention_bwd_dkv_kernel")


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    return p


def cabi_bwd(pkg, qkv, dout, n_head):
    """forward (out, lse) then spq_causal_attention_bwd on device tensors -> dqkv [B, T, 3C], pre-filled with NaN"""
    B, T, C3 = qkv.shape
    d = C3 // 3 // n_head
    L = pkg._lib
    lib = L.load()
    out, lse = pkg.causal_attention(qkv, n_head, return_lse=True)
    dqkv = torch.full_like(qkv, float("nan"))
    nbytes = lib.spq_causal_attention_bwd_workspace_bytes(B, T, n_head, d)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)
    rc = lib.spq_causal_attention_bwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), dout.data_ptr(), B, T, n_head, d,
                                      dqkv.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr(qkv.device))
    L.check(rc, "spq_causal_attention_bwd")
    return dqkv


def run_case(pkg, B, T, H, d, scale=1.0, offset=0.0, seed=None):
    qkv, dout, g64, g32 = cached_case(B, T, H, d, scale, offset, B * 1000 + T if seed is None else seed)
    return cabi_bwd(pkg, qkv.to(DEV), dout.to(DEV), H), g32, g64


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 2, 64, 1.0), (2, 63, 2, 64, 1.0), (2, 64, 2, 64, 1.0), (1, 65, 2, 64, 1.0), (2, 129, 3, 64, 1.0),
          (2, 200, 3, 64, 1.0), (1, 257, 2, 64, 1.0), (1, 257, 2, 64, 2.0), (3, 77, 4, 32, 1.0), (2, 65, 5, 16, 1.0),
          (1, 1024, 2, 64, 1.0)]


@pytest.mark.parametrize("B,T,H,d,scale", SHAPES)
def test_parity(pkg, B, T, H, d, scale):
    got, g32, g64 = run_case(pkg, B, T, H, d, scale)
    assert not bool(torch.isnan(got).any())                                     # every element was written
    judge_thirds(got, g32, g64, f"B{B} T{T} {H}x{d} x{scale:g}", standard=True)


def test_single_position_is_exact(pkg):
    """T = 1: the only probability is 1, so dq = dk = 0 and dv = dout, bit for bit"""
    qkv, dout, _, _ = cached_case(1, 1, 2, 64, 1.0, 0.0, 1001)
    got = cabi_bwd(pkg, qkv.to(DEV), dout.to(DEV), 2).cpu()
    C = 128
    assert not bool(got[..., :2 * C].any()) and torch.equal(got[..., 2 * C:], dout)


@pytest.mark.parametrize("scale,offset", [(1.0, 2.0), (3.0, 0.0)])
def test_stress_inputs_are_reported_only(pkg, scale, offset):
    """offset + 2 and randn x 3: the fp32 CPU autograd itself leaves the bar here, so the figures are printed, not asserted"""
    got, g32, g64 = run_case(pkg, 1, 257, 2, 64, scale, offset, seed=7)
    assert not bool(torch.isnan(got).any())
    judge_thirds(got, g32, g64, f"stress x{scale:g} +{offset:g}", standard=False, check=False)


# ---- 2. properties -----------------------------------------------------------------------------------------------------------
def test_runs_repeat(pkg):
    qkv, dout = (t.to(DEV) for t in make_case(3, 333, 3, 64, seed=21))
    a = cabi_bwd(pkg, qkv, dout, 3)
    b = cabi_bwd(pkg, qkv, dout, 3)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())


def test_batch_invariance(pkg):
    qkv, dout = (t.to(DEV) for t in make_case(4, 300, 3, 64, seed=22))
    full = cabi_bwd(pkg, qkv, dout, 3)
    for part in (slice(0, 2), slice(2, 4)):
        assert torch.equal(cabi_bwd(pkg, qkv[part].contiguous(), dout[part].contiguous(), 3), full[part])
    perm = torch.tensor([2, 0, 3, 1], device=DEV)
    assert torch.equal(cabi_bwd(pkg, qkv[perm].contiguous(), dout[perm].contiguous(), 3), full[perm])


@pytest.mark.parametrize("Tp", [33, 77])
def test_zero_tail(pkg, Tp):
    """dout rows >= T' zero: rows < T' of dq | dk | dv are the T'-long call bit for bit, and dq is exactly zero from T' on"""
    T, H, d = 100, 3, 64
    qkv, dout = (t.to(DEV) for t in make_case(2, T, H, d, seed=23))
    dout[:, Tp:] = 0
    full = cabi_bwd(pkg, qkv, dout, H)
    short = cabi_bwd(pkg, qkv[:, :Tp].contiguous(), dout[:, :Tp].contiguous(), H)
    assert torch.equal(full[:, :Tp], short)
    assert not bool(full[:, Tp:, :H * d].any())


def test_head_independence(pkg):
    """a NaN in one q row of (sequence 1, head 2) leaves every other (sequence, head) bit-identical to the clean run"""
    B, T, H, d = 2, 150, 3, 64
    C = H * d
    qkv, dout = (t.to(DEV) for t in make_case(B, T, H, d, seed=24))
    clean = cabi_bwd(pkg, qkv, dout, H)
    dirty_in = qkv.clone()
    dirty_in[1, 40, 2 * d + 5] = float("nan")
    dirty = cabi_bwd(pkg, dirty_in, dout, H)
    per_head = lambda t: t.view(B, T, 3, H, d)
    keep = torch.ones(B, H, dtype=torch.bool)
    keep[1, 2] = False
    for b in range(B):
        for h in range(H):
            same = torch.equal(per_head(dirty)[b, :, :, h], per_head(clean)[b, :, :, h])
            assert same == bool(keep[b, h]), (b, h)
    assert bool(torch.isnan(per_head(dirty)[1, 40, 0, 2]).any())


# ---- 3. the Python path ------------------------------------------------------------------------------------------------------
def _launched(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def _has(names, kernel):
    return any(kernel in n for n in names)


def test_autograd_entry_point(pkg):
    H = 3
    qkv, dout = (t.to(DEV) for t in make_case(2, 130, H, 64, seed=26))
    want = cabi_bwd(pkg, qkv, dout, H)
    x = qkv.clone().requires_grad_(True)
    out = pkg.causal_attention_autograd(x, H)
    assert torch.equal(out, pkg.causal_attention(qkv, H)) and out.grad_fn is not None
    out.backward(dout)
    assert torch.equal(x.grad, want)
    # a non-contiguous incoming gradient
    x2 = qkv.clone().requires_grad_(True)
    g_nc = dout.transpose(1, 2).contiguous().transpose(1, 2)
    assert not g_nc.is_contiguous()
    pkg.causal_attention_autograd(x2, H).backward(g_nc)
    assert torch.equal(x2.grad, want)
    # a gradient that arrives through a cast
    x3 = qkv.clone().requires_grad_(True)
    (pkg.causal_attention_autograd(x3, H).double() * dout.double()).sum().backward()
    assert torch.equal(x3.grad, want)
    with pytest.raises(ValueError):
        pkg.causal_attention_autograd(make_case(1, 8, 2, 80)[0].to(DEV).requires_grad_(True), 2)    # forward-only head size


def test_double_backward_raises(pkg):
    x = make_case(1, 40, 2, 64, seed=27)[0].to(DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(pkg.causal_attention_autograd(x, 2).square().sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def test_no_gradient_needed_launches_no_backward(pkg):
    qkv = make_case(1, 70, 2, 64, seed=28)[0].to(DEV)
    w = torch.ones(1, device=DEV, requires_grad=True)
    out = pkg.causal_attention_autograd(qkv, 2)
    assert out.grad_fn is None
    names = _launched(lambda: (pkg.causal_attention_autograd(qkv, 2) * w).sum().backward())
    assert _has(names, FWD_KERNEL) and not any(_has(names, k) for k in BWD_KERNELS), names
    with torch.no_grad():
        assert pkg.causal_attention_autograd(qkv.clone().requires_grad_(True), 2).grad_fn is None


def test_checkpoint_gives_the_same_gradient(pkg):
    from torch.utils.checkpoint import checkpoint
    H = 2
    qkv, dout = (t.to(DEV) for t in make_case(2, 90, H, 64, seed=29))
    a = qkv.clone().requires_grad_(True)
    pkg.causal_attention_autograd(a, H).backward(dout)
    b = qkv.clone().requires_grad_(True)
    checkpoint(lambda t: pkg.causal_attention_autograd(t, H), b, use_reentrant=False).backward(dout)
    assert torch.equal(a.grad, b.grad)


def test_stream_capture_replays(pkg):
    H = 3
    qkv, dout = (t.to(DEV) for t in make_case(2, 257, H, 64, seed=30))
    want = cabi_bwd(pkg, qkv, dout, H)
    x = qkv.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # warm-up on the capture stream (its workspace)
        torch.autograd.grad(pkg.causal_attention_autograd(x, H), x, dout)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        (grad,) = torch.autograd.grad(pkg.causal_attention_autograd(x, H), x, dout)
    for _ in range(2):
        grad.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(grad, want)
    new_qkv, new_dout = (t.to(DEV) for t in make_case(2, 257, H, 64, seed=31))   # new contents, same addresses
    with torch.no_grad():
        x.copy_(new_qkv)
    dout.copy_(new_dout)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(grad, cabi_bwd(pkg, new_qkv, new_dout, H))


# ---- 4. the modules ----------------------------------------------------------------------------------------------------------
def _config(bits=4, r=16, E=256, H=4, T=256):
    return types.SimpleNamespace(n_embd=E, n_head=H, n_positions=T, layer_norm_epsilon=1e-5, bit_widths=[bits, 32],
                                 lora_rank_per_bit={bits: r, 32: 0}, lora_alpha_per_bit={bits: 2 * r, 32: 0},
                                 quantizer_per_bit={bits: "minmax", 32: None}, per_channel_quantization=True)


def _block(pkg, bits=4, E=256, H=4, T=256):
    torch.manual_seed(0)
    blk = pkg.SPBlock(_config(bits, 16, E, H, T), bit_widths=[bits, 32])
    with torch.no_grad():
        for n, p_ in blk.named_parameters():
            if "lora_B" in n:
                p_.copy_(0.02 * torch.randn_like(p_))
    return blk


def test_core_with_both_flags(pkg):
    B, T, H, d = 2, 200, 4, 64
    qkv, dout, g64, g32 = cached_case(B, T, H, d, 1.0, 0.0, 41)
    torch.manual_seed(0)
    att = pkg.SPAttention(_config(E=H * d, H=H, T=T), [4, 32]).to(DEV)

    def run(core, backward=False):
        pkg.set_attention_core(att, core, backward=backward)
        x = qkv.to(DEV).requires_grad_(True)
        names = _launched(lambda: att.core(x).backward(dout.to(DEV)))
        return names, x.grad
    run("sdpa")                                                                 # untimed first run: one-time launches stay out
    names_sdpa, _ = run("sdpa")
    names_exp, _ = run("explicit")
    names_hip, grad = run("hip", backward=True)
    sdpa_only = set(names_sdpa) - set(names_exp)
    print(f"[attention bwd] core: SDPA-only kernels {sorted(sdpa_only)}")
    assert sdpa_only, names_sdpa
    assert _has(names_hip, FWD_KERNEL) and all(_has(names_hip, k) for k in BWD_KERNELS), names_hip
    assert not (sdpa_only & set(names_hip)), sdpa_only & set(names_hip)
    assert not any(_has(names_sdpa + names_exp, k) for k in (FWD_KERNEL,) + BWD_KERNELS)
    judge_thirds(grad, g32, g64, "SPAttention.core, both flags", standard=True)
    names_fwd_only, _ = run("hip")                                              # without the backward flag: SDPA, as before
    assert sdpa_only <= set(names_fwd_only) and not any(_has(names_fwd_only, k) for k in (FWD_KERNEL,) + BWD_KERNELS)


def test_block_at_32_bits(pkg):
    """No quantizer at 32 bits (plain F.linear), so no level can flip: every gradient of the block is judged against a float64
    CPU copy of the block on the explicit core, with e_ref the SDPA run's own err/bound."""
    E, H, T, B = 256, 4, 256, 2
    blk = _block(pkg, 4, E, H, T)
    blk.set_precision(32)
    blk.train()
    x_cpu = torch.randn(B, T, E, generator=torch.Generator().manual_seed(3))
    ref = copy.deepcopy(blk).double()
    pkg.set_attention_core(ref, "explicit")
    x64 = x_cpu.double().requires_grad_(True)
    ref(x64).square().sum().backward()
    want = {"x": x64.grad}
    want.update({n: p_.grad for n, p_ in ref.named_parameters() if p_.grad is not None})
    blk = blk.to(DEV)

    def grads(core, backward=False):
        pkg.set_attention_core(blk, core, backward=backward)
        blk.zero_grad(set_to_none=True)
        x = x_cpu.to(DEV).requires_grad_(True)
        names = _launched(lambda: blk(x).square().sum().backward())
        got = {"x": x.grad}
        got.update({n: p_.grad for n, p_ in blk.named_parameters() if p_.grad is not None})
        return names, got
    _, g_sdpa = grads("sdpa")
    names, g_hip = grads("hip", backward=True)
    pkg.set_attention_core(blk, "sdpa")
    assert _has(names, FWD_KERNEL) and all(_has(names, k) for k in BWD_KERNELS), names
    assert set(g_hip) == set(g_sdpa) == set(want) and len(want) > 8
    for n in want:
        judge_tensor(g_hip[n], g_sdpa[n], want[n], f"SPBlock 32-bit {n}", standard=False)


def test_block_at_4_bits_base_frozen(pkg):
    bits, E, H, T = 4, 256, 4, 256
    blk = _block(pkg, bits, E, H, T).to(DEV).eval()
    g = torch.Generator().manual_seed(2)
    x0, x1, x2 = (torch.randn(2, T, E, generator=g).to(DEV) for _ in range(3))
    pkg.calibrate_model(blk, bits, [x0, x1])
    blk.train()
    for lin in (blk.attn.c_attn, blk.attn.c_proj, blk.mlp.c_fc, blk.mlp.c_proj):     # base weights frozen (main_sp.py:83)
        lin.linear.weight.requires_grad_(False)
        lin.linear.bias.requires_grad_(False)
    pkg.set_attention_core(blk, "hip", backward=True)

    def step():
        blk.zero_grad(set_to_none=True)
        x = x2.clone().requires_grad_(True)
        names = _launched(lambda: blk(x).square().sum().backward())
        return names, [x.grad] + [p_.grad for p_ in blk.parameters() if p_.grad is not None]
    step()                                                                      # one-time launches (operand caches)
    names, g1 = step()
    _, g2 = step()
    pkg.set_attention_core(blk, "sdpa")
    assert _has(names, FWD_KERNEL) and all(_has(names, k) for k in BWD_KERNELS), names
    assert len(g1) == len(g2) > 1
    for a, b in zip(g1, g2):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)


def test_unserved_head_size_takes_the_old_path(pkg):
    """head_dim 48 (E = 192, H = 4): both flags on change nothing -- no kernel of the library's core, the flags-off gradients"""
    E, H, T = 192, 4, 64
    blk = _block(pkg, 4, E, H, T)
    blk.set_precision(32)
    blk = blk.to(DEV).train()
    x_dev = torch.randn(2, T, E, generator=torch.Generator().manual_seed(4)).to(DEV)

    def grads(core, backward=False):
        pkg.set_attention_core(blk, core, backward=backward)
        blk.zero_grad(set_to_none=True)
        x = x_dev.clone().requires_grad_(True)
        names = _launched(lambda: blk(x).square().sum().backward())
        return names, [x.grad] + [p_.grad for p_ in blk.parameters() if p_.grad is not None]
    _, g_off = grads("sdpa")
    names, g_on = grads("hip", backward=True)
    pkg.set_attention_core(blk, "sdpa")
    assert not any(_has(names, k) for k in (FWD_KERNEL,) + BWD_KERNELS), names
    assert len(g_on) == len(g_off) > 1
    for a, b in zip(g_on, g_off):
        assert torch.equal(a, b)
