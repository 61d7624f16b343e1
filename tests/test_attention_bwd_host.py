"""No GPU: the C ABI of the causal attention backward (declaration, export, refusals decided on the host, the workspace size)
and the ``SPAttention.use_hip_backward`` switch on tensors the kernels do not serve."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    import llm_qat_on_gpt2_amd as p
    if not os.path.exists(p._lib.LIB_PATH):
        g.build()
    p._lib.load()
    return p


def test_declared_exported_and_bound(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spq.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+spq_causal_attention_bwd\s*\(\s*const float\*\s*qkv\s*,\s*const float\*\s*out\s*,\s*const float\*\s*lse\s*,"
                     r"\s*const float\*\s*dout\s*,\s*int64_t B\s*,\s*int64_t T\s*,\s*int64_t n_head\s*,\s*int64_t head_dim\s*,"
                     r"\s*float\*\s*dqkv\s*,\s*void\*\s*workspace\s*,\s*size_t workspace_bytes\s*,\s*spq_stream_t stream\s*\)\s*;", src)
    assert re.search(r"\bint64_t\s+spq_causal_attention_bwd_workspace_bytes\s*\(\s*int64_t B\s*,\s*int64_t T\s*,\s*int64_t n_head\s*,"
                     r"\s*int64_t head_dim\s*\)\s*;", src)
    lib = pkg._lib.load()
    for name in ("spq_causal_attention_bwd", "spq_causal_attention_bwd_workspace_bytes"):
        assert hasattr(lib, name) and name in pkg._lib.SIGNATURES
    assert pkg.causal_attention_autograd is pkg.attention.causal_attention_autograd
    assert pkg.attention.BWD_HEAD_DIMS == (16, 32, 64) and set(pkg.attention.BWD_HEAD_DIMS) <= set(pkg.attention.HEAD_DIMS)
    assert not pkg.attention.served_backward(torch.zeros(1, 4, 192), 1)                 # a CPU tensor is never served


# made up, 16-byte aligned; nothing dereferences them
QKV, OUT, LSE, DOUT, DQKV, WS = (0x7000_0000_0000 + i * 0x0100_0000_0000 for i in range(6))


def _call(lib, qkv=QKV, out=OUT, lse=LSE, dout=DOUT, B=2, T=16, H=4, d=64, dqkv=DQKV, ws=WS, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(int(lib.spq_causal_attention_bwd_workspace_bytes(B, T, H, d)), 0)
    return lib.spq_causal_attention_bwd(qkv, out, lse, dout, B, T, H, d, dqkv, ws, ws_bytes, None)


@pytest.mark.parametrize("kw,word", [
    (dict(d=48), b"head_dim"),
    (dict(d=80), b"head_dim"),
    (dict(T=0), b"at least 1"),
    (dict(B=0), b"at least 1"),
    (dict(H=0), b"at least 1"),
    (dict(dqkv=DQKV + 4), b"16-byte aligned"),
    (dict(dout=DOUT + 8), b"16-byte aligned"),
    (dict(ws=WS + 4), b"16-byte aligned"),
    (dict(ws_bytes=2 * 4 * 16 * 4 - 1), b"workspace too small"),
    (dict(ws_bytes=0), b"workspace too small"),
    (dict(B=1 << 20, T=1 << 20, H=64, ws_bytes=1 << 40), b"too large"),
])
def test_refusals_precede_every_launch(pkg, kw, word):
    """Decided before any device call: without a device a launch attempt would come back as SPQ_ERR_LAUNCH (-2).  The addresses are
    made up, so this runs only where no launch can succeed."""
    if torch.cuda.is_available():
        pytest.skip("made-up operand addresses: only where no launch can succeed")
    lib = pkg._lib.load()
    rc = _call(lib, **kw)
    assert rc == UNSUPPORTED, (rc, lib.spq_last_error())
    assert word in lib.spq_last_error() and b"spq_causal_attention_bwd:" in lib.spq_last_error(), lib.spq_last_error()


@pytest.mark.parametrize("which", ["qkv", "out", "lse", "dout", "dqkv", "ws"])
def test_null_pointers_are_invalid(pkg, which):
    lib = pkg._lib.load()
    assert _call(lib, ws_bytes=512, **{which: None}) == INVALID
    assert b"null pointer" in lib.spq_last_error()


def test_workspace_bytes_agrees_with_the_refusals(pkg):
    lib = pkg._lib.load()
    f = lib.spq_causal_attention_bwd_workspace_bytes
    for d in pkg.attention.BWD_HEAD_DIMS:
        n = f(2, 16, 4, d)
        assert n >= 2 * 16 * 4 * 4 and n % 16 == 0                                      # delta [B, H, T] in fp32
    assert f(3, 77, 5, 64) >= 3 * 77 * 5 * 4 and f(3, 77, 5, 64) % 16 == 0
    for args, word in (((2, 16, 4, 48), b"head_dim"), ((2, 16, 4, 128), b"head_dim"), ((2, 0, 4, 64), b"at least 1"),
                       ((0, 16, 4, 64), b"at least 1"), ((2, 16, 0, 64), b"at least 1"), ((1 << 20, 1 << 20, 64, 64), b"too large")):
        assert f(*args) == UNSUPPORTED, args
        assert word in lib.spq_last_error(), lib.spq_last_error()
    if not torch.cuda.is_available():                                                   # (made-up addresses, as above)
        n = f(2, 16, 4, 64)
        assert _call(lib, ws_bytes=2 * 16 * 4 * 4 - 4) == UNSUPPORTED                   # one float short: refused on the host
        assert _call(lib, ws_bytes=n) not in (UNSUPPORTED, INVALID)                     # enough: past validation (no device: -2)


def _attention(pkg, E=64, H=4):
    cfg = types.SimpleNamespace(n_embd=E, n_head=H, n_positions=32, layer_norm_epsilon=1e-5, bit_widths=[4, 32],
                                lora_rank_per_bit={4: 4, 32: 0}, lora_alpha_per_bit={4: 8, 32: 0},
                                quantizer_per_bit={4: "minmax", 32: None}, per_channel_quantization=True)
    torch.manual_seed(0)
    return pkg.SPAttention(cfg, [4, 32]).eval()


def test_flag_is_off_by_default_and_the_helper_sets_it(pkg):
    att = _attention(pkg)
    assert att.use_hip_backward is False and att.use_hip_core is False
    holder = torch.nn.ModuleList([att, _attention(pkg)])
    assert pkg.set_attention_core(holder, "hip", backward=True) == 2
    assert all(m.use_hip_core and m.use_hip_backward and m.use_sdpa for m in holder)
    assert pkg.set_attention_core(holder, "hip") == 2 and all(m.use_hip_core and not m.use_hip_backward for m in holder)
    for core in ("sdpa", "explicit"):
        pkg.set_attention_core(holder, "hip", backward=True)
        assert pkg.set_attention_core(holder, core) == 2 and not any(m.use_hip_backward or m.use_hip_core for m in holder)
        assert pkg.set_attention_core(holder, core, backward=True) == 2 and not any(m.use_hip_backward for m in holder)


def test_both_flags_change_nothing_on_a_cpu_tensor_with_a_gradient(pkg):
    att = _attention(pkg)
    qkv = torch.randn(3, 24, 192, generator=torch.Generator().manual_seed(1))
    a = qkv.clone().requires_grad_(True)
    ya = att.core(a)
    ya.square().sum().backward()
    att.use_hip_core = att.use_hip_backward = True
    b = qkv.clone().requires_grad_(True)
    yb = att.core(b)
    assert yb.grad_fn is not None
    yb.square().sum().backward()
    assert torch.equal(ya, yb) and torch.equal(a.grad, b.grad)


def test_python_entry_point_refuses_cpu_tensors(pkg):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.causal_attention_autograd(torch.zeros(1, 4, 192, requires_grad=True), 1)
