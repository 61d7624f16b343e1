"""No GPU: the C ABI of the LM cross-entropy pair (declarations, exports, refusals decided on the host), the Python names, the
``SPLMHeadModel.use_hip_loss`` switch on tensors the kernels do not serve, and the yardstick's own error (tests/lm_loss_ref.py)."""
import os
import re
import types

import pytest
import torch

from lm_loss_ref import E_REF_LIMIT, FAMILIES, make_labels, make_logits, yardstick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -3
FWD, BWD = "spq_lm_cross_entropy_fwd", "spq_lm_cross_entropy_bwd"


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
    assert re.search(r"\bint\s+spq_lm_cross_entropy_fwd\s*\(\s*const float\*\s*logits\s*,\s*const int64_t\*\s*labels\s*,\s*int64_t B\s*,"
                     r"\s*int64_t T\s*,\s*int64_t V\s*,\s*int shift\s*,\s*int64_t ignore_index\s*,\s*float\*\s*nll\s*,\s*float\*\s*lse\s*,"
                     r"\s*float\*\s*loss\s*,\s*int64_t\*\s*count\s*,\s*spq_stream_t stream\s*\)\s*;", src)
    assert re.search(r"\bint\s+spq_lm_cross_entropy_bwd\s*\(\s*const float\*\s*logits\s*,\s*const int64_t\*\s*labels\s*,"
                     r"\s*const float\*\s*lse\s*,\s*int64_t B\s*,\s*int64_t T\s*,\s*int64_t V\s*,\s*int shift\s*,\s*int64_t ignore_index\s*,"
                     r"\s*const float\*\s*grad\s*,\s*const float\*\s*grad_per_row\s*,\s*const int64_t\*\s*count\s*,\s*float\*\s*dlogits\s*,"
                     r"\s*spq_stream_t stream\s*\)\s*;", src)
    lib = pkg._lib.load()
    for name in (FWD, BWD):
        assert hasattr(lib, name) and name in pkg._lib.SIGNATURES
    assert pkg.lm_cross_entropy is pkg.lm_loss.lm_cross_entropy and pkg.token_nll is pkg.lm_loss.token_nll
    assert pkg.set_lm_loss is pkg.blocks.set_lm_loss
    assert {"lm_cross_entropy", "token_nll", "set_lm_loss"} <= set(pkg.__all__)
    assert pkg.lm_loss.PLAN_CHANGES == (4, 1028, 2052, 3076, 4100, 8196)
    assert pkg.lm_loss.plan_boundaries(50257) == (4, 256, 1024, 4096, 50256) and pkg.lm_loss.plan_boundaries(3) == ()


# made up, 16-byte aligned; nothing dereferences them
LOGITS, LABELS, LSE, NLL, LOSS, COUNT, GRAD, DLOGITS = (0x7000_0000_0000 + i * 0x0100_0000_0000 for i in range(8))


def _fwd(lib, logits=LOGITS, labels=LABELS, B=2, T=9, V=257, shift=1, nll=NLL, lse=LSE, loss=LOSS, count=COUNT):
    return lib.spq_lm_cross_entropy_fwd(logits, labels, B, T, V, shift, -100, nll, lse, loss, count, None)


def _bwd(lib, logits=LOGITS, labels=LABELS, lse=LSE, B=2, T=9, V=257, shift=1, grad=GRAD, grad_per_row=None, count=COUNT,
         dlogits=DLOGITS):
    return lib.spq_lm_cross_entropy_bwd(logits, labels, lse, B, T, V, shift, -100, grad, grad_per_row, count, dlogits, None)


REFUSALS = [
    (dict(V=0), b"at least 1"),
    (dict(B=0), b"at least 1"),
    (dict(T=0), b"at least 1"),
    (dict(logits=LOGITS + 2), b"logits"),
    (dict(labels=LABELS + 4), b"labels"),
    (dict(B=1 << 20, T=1 << 20), b"too large"),
    (dict(V=1 << 31), b"too large"),
    (dict(shift=2), b"shift"),
]


@pytest.mark.parametrize("call,name", [(_fwd, FWD), (_bwd, BWD)], ids=["fwd", "bwd"])
@pytest.mark.parametrize("kw,word", REFUSALS + [(dict(count=COUNT + 4), b"count")])
def test_refusals_precede_every_launch(pkg, call, name, kw, word):
    """Decided before any device call: without a device a launch attempt would come back as SPQ_ERR_LAUNCH (-2).  The addresses are
    made up, so this runs only where no launch can succeed."""
    if torch.cuda.is_available():
        pytest.skip("made-up operand addresses: only where no launch can succeed")
    lib = pkg._lib.load()
    rc = call(lib, **kw)
    assert rc == UNSUPPORTED, (rc, lib.spq_last_error())
    assert word in lib.spq_last_error() and name.encode() + b":" in lib.spq_last_error(), lib.spq_last_error()


def test_further_refusals_and_a_call_that_passes_validation(pkg):
    if torch.cuda.is_available():
        pytest.skip("made-up operand addresses: only where no launch can succeed")
    lib = pkg._lib.load()
    assert _bwd(lib, dlogits=DLOGITS + 2) == UNSUPPORTED and b"dlogits" in lib.spq_last_error()
    assert _bwd(lib, grad_per_row=GRAD) == UNSUPPORTED and b"exclude" in lib.spq_last_error()
    # 4-byte alignment of logits / dlogits and 8-byte alignment of labels is all that is asked: past validation (no device: -2)
    assert _fwd(lib, logits=LOGITS + 4, labels=LABELS + 8) not in (UNSUPPORTED, INVALID)
    assert _bwd(lib, logits=LOGITS + 12, dlogits=DLOGITS + 4, count=None) not in (UNSUPPORTED, INVALID)
    assert _bwd(lib, grad=None, grad_per_row=GRAD, count=None) not in (UNSUPPORTED, INVALID)
    assert _fwd(lib, T=1) not in (UNSUPPORTED, INVALID)                                  # T = 1 under the shift is served


@pytest.mark.parametrize("which", ["logits", "labels", "nll", "lse", "loss", "count"])
def test_forward_null_pointers_are_invalid(pkg, which):
    lib = pkg._lib.load()
    assert _fwd(lib, **{which: None}) == INVALID
    assert b"null pointer" in lib.spq_last_error() and which.encode() in lib.spq_last_error() and FWD.encode() in lib.spq_last_error()


@pytest.mark.parametrize("which", ["logits", "labels", "lse", "dlogits", "grad"])
def test_backward_null_pointers_are_invalid(pkg, which):
    lib = pkg._lib.load()
    assert _bwd(lib, **{which: None}) == INVALID                                         # grad: neither grad nor grad_per_row
    assert b"null pointer" in lib.spq_last_error() and which.encode() in lib.spq_last_error() and BWD.encode() in lib.spq_last_error()


def test_served_is_false_off_the_kernels_domain_and_the_functions_raise(pkg):
    x, y = torch.zeros(2, 5, 7), torch.zeros(2, 5, dtype=torch.int64)
    assert not pkg.lm_loss.served(x, y)                                                  # CPU tensors are never served
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.lm_cross_entropy(x, y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.token_nll(x, y)
    with pytest.raises(ValueError, match="reduction"):
        pkg.lm_cross_entropy(x, y, reduction="batchmean")


def _model(pkg):
    cfg = types.SimpleNamespace(vocab_size=37, n_positions=16, n_embd=32, n_layer=1, n_head=2, layer_norm_epsilon=1e-5,
                                embd_pdrop=0.0, bit_widths=[4, 32], lora_rank_per_bit={4: 4, 32: 0}, lora_alpha_per_bit={4: 8, 32: 0},
                                quantizer_per_bit={4: "minmax", 32: None}, per_channel_quantization=True)
    torch.manual_seed(0)
    model = pkg.SPLMHeadModel(cfg)
    model.set_precision(32)
    return model


def test_flag_is_off_by_default_and_the_helper_sets_it(pkg):
    holder = torch.nn.ModuleList([_model(pkg), _model(pkg)])
    assert all(m.use_hip_loss is False for m in holder)
    assert pkg.set_lm_loss(holder, "hip") == 2 and all(m.use_hip_loss is True for m in holder)
    assert pkg.set_lm_loss(holder, "torch") == 2 and not any(m.use_hip_loss for m in holder)
    assert pkg.set_lm_loss(holder[0].transformer, "hip") == 0
    with pytest.raises(ValueError, match="hip"):
        pkg.set_lm_loss(holder, "triton")


def test_flag_changes_nothing_on_cpu_tensors(pkg):
    model = _model(pkg)
    ids = torch.randint(37, (2, 12), generator=torch.Generator().manual_seed(1))

    def step():
        model.zero_grad(set_to_none=True)
        out = model(ids, labels=ids)
        out["loss"].backward()
        return out, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    off, g_off = step()
    pkg.set_lm_loss(model, "hip")
    on, g_on = step()
    assert torch.equal(off["loss"], on["loss"]) and torch.equal(off["logits"], on["logits"])
    assert set(g_off) == set(g_on) and len(g_off) > 4 and all(torch.equal(g_off[n], g_on[n]) for n in g_off)


@pytest.mark.parametrize("V", [3, 65, 257, 4099, 50257])
def test_the_fp32_reference_is_a_fit_yardstick(V):
    """On every input family at (B, T) = (2, 9) the reference's own fp32 run stays within 0.15 of the bar against float64, on the
    per-row NLL, the scalar loss and dlogits: the allowance 1 + e_ref of the GPU tests is at most 1.15 there."""
    for family in FAMILIES:
        for shift in (True, False):
            _, e_ref = yardstick(make_logits(family, 2, 9, V, seed=V), make_labels(2, 9, V, seed=V), shift=shift)
            assert max(e_ref[k] for k in ("nll", "sum", "mean", "dlogits")) <= E_REF_LIMIT, (family, shift, e_ref)
