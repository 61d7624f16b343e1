"""CPU: the C ABI of the SwitchableLayerNorm backward (symbols, workspace size = the scheduling-independent slab cut) and the
module's dispatch where the HIP pair must NOT be taken."""
import json
import os
import re

import numpy as np
import pytest
import torch

import ln_grad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("spq_layernorm_fwd_stats", "spq_layernorm_bwd_workspace_bytes", "spq_layernorm_bwd")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    import llm_qat_on_gpt2_amd as p
    if not os.path.exists(p._lib.LIB_PATH):
        g.build()
    p._lib.load()
    return p


def test_new_entry_points_declared_and_exported(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "spq.h")).read(), flags=re.S)
    lib = pkg._lib.load()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, src), f"{n} is not declared in include/spq.h"
        assert n in pkg._lib.SIGNATURES, f"{n} has no ctypes signature"
        assert hasattr(lib, n), f"{n} is not exported by libspq.so"


def test_workspace_is_the_slab_cut(pkg):
    """S slabs x {dweight, dbias} x cols floats, with S = min(512, ceil(rows / 16)) a function of rows alone (closed form:
    at most 512 * 2 * cols * 4 bytes), slab s = rows [s rows / S, (s + 1) rows / S)."""
    f = pkg._lib.load().spq_layernorm_bwd_workspace_bytes
    for cols in (4, 64, 68, 768, 1024, 3072, 8192):
        prev = 0
        for rows in (1, 3, 4, 5, 15, 16, 17, 64, 4099, 8191, 8192, 8193, 8208, 32768, 100000, 1 << 22):
            n = f(rows, cols)
            S = R.slabs(rows)
            assert n == S * 2 * cols * 4, (rows, cols, n, S)
            assert 0 < n <= 512 * 2 * cols * 4
            assert n >= prev and n == f(rows, cols)
            assert n % 16 == 0
            prev = n
    assert R.slabs(8192) == 512 and R.slabs(32768) == 512 and R.slabs(4099) == 257 and R.slabs(17) == 2 and R.slabs(1) == 1
    for rows in (1, 17, 4099, 8193, 32768):                 # the slabs tile the rows, none empty
        cut = [R.slab_range(rows, s) for s in range(R.slabs(rows))]
        assert cut[0][0] == 0 and cut[-1][1] == rows and all(a[1] == b[0] for a, b in zip(cut, cut[1:]))
        assert all(0 < b - a <= -(-rows // R.slabs(rows)) for a, b in cut)
    for rows, cols in ((0, 768), (-1, 768), (8, 0), (8, 6), (8, 8196)):
        assert f(rows, cols) == 0


def test_refusals_precede_every_launch(pkg):
    """Without a device a launch attempt would come back as SPQ_ERR_LAUNCH (-2); made-up addresses, so only where none can succeed."""
    if torch.cuda.is_available():
        pytest.skip("made-up operand addresses: only where no launch can succeed")
    lib = pkg._lib.load()
    a = [0x7000_0000_0000 + i * 0x1000_0000 for i in range(10)]
    big = 1 << 40
    assert lib.spq_layernorm_fwd_stats(a[0], 8, 768, a[1], a[2], 1e-5, a[3], None, a[5], None) == -1
    assert b"null pointer" in lib.spq_last_error()
    assert lib.spq_layernorm_fwd_stats(a[0], 8, 6, a[1], a[2], 1e-5, a[3], a[4], a[5], None) == -3
    assert lib.spq_layernorm_bwd(None, a[1], a[2], a[3], a[4], 8, 768, a[5], a[6], a[7], a[8], big, None) == -1
    assert lib.spq_layernorm_bwd(a[0], a[1], a[2], a[3], a[4], 8, 768, None, None, None, a[8], big, None) == -1
    assert lib.spq_layernorm_bwd(a[0], a[1], a[2], a[3], a[4], 0, 768, a[5], a[6], a[7], a[8], big, None) == -1
    assert b"empty" in lib.spq_last_error()
    for cols in (6, 8196):
        assert lib.spq_layernorm_bwd(a[0], a[1], a[2], a[3], a[4], 8, cols, a[5], a[6], a[7], a[8], big, None) == -3
        assert b"cols" in lib.spq_last_error()
    assert lib.spq_layernorm_bwd(a[0] + 4, a[1], a[2], a[3], a[4], 8, 768, a[5], a[6], a[7], a[8], big, None) == -3
    need = lib.spq_layernorm_bwd_workspace_bytes(8, 768)
    assert lib.spq_layernorm_bwd(a[0], a[1], a[2], a[3], a[4], 8, 768, a[5], a[6], a[7], a[8], need - 1, None) == -5
    assert b"workspace" in lib.spq_last_error()


@pytest.mark.parametrize("how", ["cpu tensor", "fuse_backward off", "2-d normalized_shape", "fp64 input"])
def test_composed_formula_where_the_kernels_do_not_apply(pkg, how, monkeypatch):
    from llm_qat_on_gpt2_amd import blocks

    def boom(*a, **k):
        raise AssertionError("the HIP autograd pair was taken")
    monkeypatch.setattr(blocks._LayerNormFunction, "apply", staticmethod(boom))
    shape = (4, 8) if how.startswith("2-d") else 8
    ln = pkg.SwitchableLayerNorm(shape, precision_levels=[4, 32])
    assert pkg.SwitchableLayerNorm.fuse_backward is (os.environ.get("SPQ_LN_AUTOGRAD", "1")[:1] != "0")
    if how == "fuse_backward off":
        ln.fuse_backward = False
    x = torch.randn(3, 4, 8, dtype=torch.float64 if how == "fp64 input" else torch.float32, requires_grad=True)
    y = ln(x)
    assert y.grad_fn is not None and y.dtype == x.dtype
    y.sum().backward()
    assert x.grad is not None and ln.weights["32"].grad is not None


@pytest.mark.parametrize("name", ["768", "1024", "64", "768_channel", "768_offset"])
def test_fixtures_are_the_oracles_autograd(name, golden_dir):
    """The fixtures hold the reference's gradients (the generator asserted the oracle's autograd equal to them bit for bit on the
    machine that wrote them).  ATen's CPU reductions do not promise one summation order across machines and thread counts, so
    here the oracle must agree with the stored values within 0.5 of the gradient bar -- two fp32 evaluations that each qualify as
    a yardstick are within 0.25 of the bar of fp64, hence within 0.5 of each other; for the offset case, whose fp32 evaluations
    sit near the bar against fp64, within twice the recorded err/bound -- and make the recorded yardstick decision."""
    with np.load(os.path.join(golden_dir, f"lngrad_{name}.npz")) as z:
        meta = json.loads(str(z["meta"]))
        t = {k: torch.from_numpy(z[k]) for k in z.files if k != "meta"}
    assert os.path.getsize(os.path.join(golden_dir, f"lngrad_{name}.npz")) < (1 << 20)
    y, dx, dw, db = R.oracle_grads(t["x"], t["g"], t["weight"], t["bias"])
    _, limit, ratio, which = R.yardstick(t["x"], t["g"], t["weight"], t["bias"])
    assert which == meta["yardstick"] and (which == "fp64") == (name == "768_offset"), (name, ratio)
    allowed = 2 * max(R.FP32_REF_LIMIT, meta["ref_ratio_vs_fp64"])
    for got, k in ((dx, "dx"), (dw, "dweight"), (db, "dbias")):
        assert R.bar_ratio(got, t[k]) <= allowed, (name, k)
    assert bool(((y.double() - t["y"].double()).abs() <= 2e-6 * t["y"].double().abs() + 2e-6).all())
