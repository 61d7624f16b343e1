"""No GPU: the C ABI of the causal attention core (declaration, export, refusals decided on the host) and the
``SPAttention.use_hip_core`` switch on tensors the kernel does not serve."""
import os
import re
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -3


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
    assert re.search(r"\bint\s+spq_causal_attention_fwd\s*\(\s*const float\*\s*qkv\s*,\s*int64_t B\s*,\s*int64_t T\s*,\s*int64_t n_head\s*,"
                     r"\s*int64_t head_dim\s*,\s*float\*\s*out\s*,\s*float\*\s*lse\s*,\s*spq_stream_t stream\s*\)\s*;", src)
    lib = pkg._lib.load()
    assert hasattr(lib, "spq_causal_attention_fwd") and "spq_causal_attention_fwd" in pkg._lib.SIGNATURES
    assert pkg.causal_attention is pkg.attention.causal_attention and callable(pkg.set_attention_core)


QKV, OUT, LSE = 0x7000_0000_0000, 0x7100_0000_0000, 0x7200_0000_0000      # made up, 16-byte aligned; nothing dereferences them


@pytest.mark.parametrize("args,word", [
    ((QKV, 2, 16, 4, 48, OUT, None), b"head_dim"),
    ((QKV, 2, 16, 4, 8, OUT, None), b"head_dim"),
    ((QKV, 2, 0, 4, 64, OUT, None), b"at least 1"),
    ((QKV, 0, 16, 4, 64, OUT, None), b"at least 1"),
    ((QKV, 2, 16, 0, 64, OUT, None), b"at least 1"),
    ((QKV + 4, 2, 16, 4, 64, OUT, None), b"16-byte aligned"),
    ((QKV, 2, 16, 4, 64, OUT + 8, None), b"16-byte aligned"),
    ((QKV, 2, 16, 4, 64, OUT, LSE + 4), b"16-byte aligned"),
    ((QKV, 1 << 20, 1 << 20, 64, 64, OUT, None), b"too large"),
])
def test_refusals_precede_every_launch(pkg, args, word):
    """Decided before any device call: without a device a launch attempt would come back as SPQ_ERR_LAUNCH (-2).  The addresses are
    made up, so this runs only where no launch can succeed."""
    if torch.cuda.is_available():
        pytest.skip("made-up operand addresses: only where no launch can succeed")
    lib = pkg._lib.load()
    rc = lib.spq_causal_attention_fwd(*args, None)
    assert rc == UNSUPPORTED, (rc, lib.spq_last_error())
    assert word in lib.spq_last_error(), lib.spq_last_error()


def test_null_pointers_are_invalid(pkg):
    lib = pkg._lib.load()
    assert lib.spq_causal_attention_fwd(None, 2, 16, 4, 64, OUT, None, None) == -1
    assert lib.spq_causal_attention_fwd(QKV, 2, 16, 4, 64, None, None, None) == -1
    assert b"null pointer" in lib.spq_last_error()


def _attention(pkg, E=64, H=4, T=24):
    cfg = types.SimpleNamespace(n_embd=E, n_head=H, n_positions=32, layer_norm_epsilon=1e-5, bit_widths=[4, 32],
                                lora_rank_per_bit={4: 4, 32: 0}, lora_alpha_per_bit={4: 8, 32: 0},
                                quantizer_per_bit={4: "minmax", 32: None}, per_channel_quantization=True)
    torch.manual_seed(0)
    return pkg.SPAttention(cfg, [4, 32]).eval()


def test_flag_is_off_by_default_and_the_helper_sets_it(pkg):
    att = _attention(pkg)
    assert att.use_hip_core is False and att.use_sdpa is True
    holder = torch.nn.ModuleList([att, _attention(pkg)])
    assert pkg.set_attention_core(holder, "hip") == 2 and all(m.use_hip_core and m.use_sdpa for m in holder)
    assert pkg.set_attention_core(holder, "explicit") == 2 and not any(m.use_hip_core or m.use_sdpa for m in holder)
    assert pkg.set_attention_core(holder, "sdpa") == 2 and all(m.use_sdpa and not m.use_hip_core for m in holder)
    with pytest.raises(ValueError):
        pkg.set_attention_core(holder, "flash")


def test_flag_changes_nothing_on_a_cpu_tensor_or_with_a_gradient(pkg):
    att = _attention(pkg)
    qkv = torch.randn(3, 24, 192, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = att.core(qkv)
        att.use_hip_core = True
        assert torch.equal(att.core(qkv), want)
    att.use_hip_core = False
    a = qkv.clone().requires_grad_(True)
    ya = att.core(a)
    ya.square().sum().backward()
    att.use_hip_core = True
    b = qkv.clone().requires_grad_(True)
    yb = att.core(b)
    assert yb.grad_fn is not None
    yb.square().sum().backward()
    assert torch.equal(ya, yb) and torch.equal(a.grad, b.grad) and torch.equal(ya.detach(), want)


def test_python_entry_point_refuses_cpu_tensors(pkg):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.causal_attention(torch.zeros(1, 4, 192), 1)
