"""GPU: the LM cross-entropy pair ``spq_lm_cross_entropy_fwd`` / ``_bwd`` (csrc/spq_lm_loss.hip) through the C ABI
-- parity of NLL, lse, sum, mean and dlogits against float64 CPU autograd at every V where the kernel's plan changes, alignment,
planted maxima, ignored / out-of-range labels, -inf entries, determinism and row independence -- then ``lm_cross_entropy``,
``token_nll``, stream capture and ``SPLMHeadModel.use_hip_loss`` (values, launch trace).

The bar (tests/lm_loss_ref.py): 1e-5 |y| + 1e-5 rms(y) against the reference's two loss lines under float64 CPU autograd, times
(1 + e_ref) with e_ref the fp32 CPU autograd's own err/bound (<= 0.15 at (B, T) = (2, 9): tests/test_lm_loss_host.py)."""
import copy
import types

import pytest
import torch

from lm_loss_ref import FAMILIES, bar_ratio, cached_case, judge, make_labels, make_logits, yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KERNELS = ("lm_cross_entropy_fwd_kernel", "lm_cross_entropy_reduce_kernel", "lm_cross_entropy_bwd_kernel")
NAN = float("nan")


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    return p


def cabi(pkg, logits, labels, shift=True, ignore_index=-100, reduction="mean", upstream=None, offset=0):
    """Both calls on device tensors, every output pre-filled with NaN -> dict(nll [B, T], lse [B, T], lse_lo, sum, mean, count,
    dlogits).  `offset`: logits and dlogits live `offset` floats past a 16-byte boundary."""
    L, lib = pkg._lib, pkg._lib.load()
    B, T, V = logits.shape
    n = B * T * V
    x = torch.empty(n + 4, dtype=torch.float32, device=DEV)
    assert x.data_ptr() % 16 == 0
    x = x[offset:offset + n].view(B, T, V).copy_(logits)
    d = torch.full((n + 4,), NAN, dtype=torch.float32, device=DEV)[offset:offset + n].view(B, T, V)
    assert x.data_ptr() % 16 == 4 * offset and d.data_ptr() % 16 == 4 * offset
    labels = labels.to(DEV)
    nll = torch.full((B, T), NAN, device=DEV)
    lse = torch.full((2, B, T), NAN, device=DEV)
    loss = torch.full((2,), NAN, device=DEV)
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    st = L.stream_ptr(x.device)
    L.check(lib.spq_lm_cross_entropy_fwd(x.data_ptr(), labels.data_ptr(), B, T, V, int(shift), ignore_index, nll.data_ptr(),
                                         lse.data_ptr(), loss.data_ptr(), count.data_ptr(), st), "spq_lm_cross_entropy_fwd")
    if upstream is None:
        upstream = torch.ones((B, T - int(shift)) if reduction == "none" else ())
    g = upstream.to(DEV).float().contiguous()
    if g.numel() == 0:                                                          # 'none' at T = 1 under the shift: never read
        g = torch.zeros(1, device=DEV)
    per_row = reduction == "none"
    L.check(lib.spq_lm_cross_entropy_bwd(x.data_ptr(), labels.data_ptr(), lse.data_ptr(), B, T, V, int(shift), ignore_index,
                                         None if per_row else g.data_ptr(), g.data_ptr() if per_row else None,
                                         count.data_ptr() if reduction == "mean" else None, d.data_ptr(), st),
            "spq_lm_cross_entropy_bwd")
    torch.cuda.synchronize()
    return dict(nll=nll, lse=lse[0], lse_lo=lse[1], sum=loss[0], mean=loss[1], count=int(count), dlogits=d)


def scored(got, shift):
    """the [B, T - shift] part of the kernel's [B, T] NLL"""
    return got["nll"][:, :got["nll"].shape[1] - int(shift)]


def judge_all(got, r64, e_ref, shift, what):
    assert not bool(torch.isnan(got["dlogits"]).any()) and not bool(torch.isnan(got["lse"]).any())   # every element was written
    out = {"nll": judge(scored(got, shift), r64, e_ref, "nll", what)}
    for key in ("lse", "sum", "mean", "dlogits"):
        out[key] = judge(got[key], r64, e_ref, key, what)
    if shift:
        assert not bool(got["dlogits"][:, -1].any()) and not bool(got["nll"][:, -1].any())             # exact zeros on the last row
    return out


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------
def parity_sizes(pkg):
    sizes = {1, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 50257}
    for v in pkg.lm_loss.PLAN_CHANGES:
        sizes |= {v - 1, v, v + 1}
    return sorted(sizes)


def test_the_plan_constant_is_the_kernels_plan(pkg):
    m = pkg.lm_loss
    assert (m.CHUNK, m.ROW_THREADS, m.CHUNKS_PER_PASS) == (4, 256, 4)
    assert m.PLAN_CHANGES == (4, 1028, 2052, 3076, 4100, 8196) and len(parity_sizes(pkg)) == 28


@pytest.mark.parametrize("V", [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 1027, 1028, 1029, 2051, 2052, 2053, 3075, 3076, 3077,
                               4099, 4100, 4101, 8195, 8196, 8197, 50257])
def test_parity(pkg, V):
    assert V in parity_sizes(pkg)
    for family in FAMILIES:
        for shift in (True, False):
            logits, labels, r64, e_ref = cached_case(family, 2, 9, V, shift, V)
            judge_all(cabi(pkg, logits, labels, shift=shift), r64, e_ref, shift, f"V={V} {family} shift={int(shift)}")
    if V == 1:                                                                  # one class: the loss and its gradient are exactly 0
        logits, labels, _, _ = cached_case("randn_x3", 2, 9, 1, False, 1)
        got = cabi(pkg, logits, labels, shift=False)
        assert not bool(got["nll"].any()) and not bool(got["dlogits"].any()) and float(got["mean"]) == 0.0


def test_parity_covers_every_plan_change(pkg):
    params = [m.args[1] for m in test_parity.pytestmark if m.name == "parametrize"][0]
    assert sorted(params) == parity_sizes(pkg)


def test_parity_at_training_width(pkg):
    """4 x 128 x 50257 with logits x 3: the fp32 reference's own gradient error is more than half of the bar here (0.56 on this
    seed; the kernel's 0.07), still inside it, so the case is asserted like every other."""
    logits, labels, r64, e_ref = cached_case("randn_x3", 4, 128, 50257, True, 11)
    judge_all(cabi(pkg, logits, labels), r64, e_ref, True, "4x128x50257 x3")


# ---- 2. alignment ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [257, 50257])
def test_every_phase_of_a_16_byte_line_gives_the_same_bits(pkg, V):
    logits, labels, r64, e_ref = cached_case("randn_x3", 2, 5, V, True, V + 1)
    want = cabi(pkg, logits, labels)
    judge_all(want, r64, e_ref, True, f"V={V} aligned")
    for offset in (1, 2, 3):
        got = cabi(pkg, logits, labels, offset=offset)
        for key in ("nll", "lse", "lse_lo", "sum", "mean", "dlogits"):
            assert torch.equal(got[key], want[key]), (offset, key)


# ---- 3. planted maxima -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [50257, 4101, 7])
def test_planted_maximum_at_every_boundary_of_the_plan(pkg, V):
    cuts = pkg.lm_loss.plan_boundaries(V)
    spots = sorted({0, V - 1} | {c - 1 for c in cuts} | set(cuts))
    assert all(0 <= s < V for s in spots) and len(spots) >= 2 * len(cuts) + 1
    T = len(spots)
    logits = make_logits("randn", 1, T, V, seed=V + 2)
    for t, s in enumerate(spots):
        logits[0, t, s] = 40.0                                                  # far above every other entry of the row
    for on in (True, False):
        labels = torch.tensor([[s if on else (s + 1) % V for s in spots]], dtype=torch.int64)
        r64, e_ref = yardstick(logits, labels, shift=False)
        got = cabi(pkg, logits, labels, shift=False)
        what = f"V={V} planted, label {'on' if on else 'off'} it"
        if on:          # NLL and gradient are ~1e-13 on every row here, below what fp32 resolves next to 1: lse and the sign only
            judge(got["lse"], r64, e_ref, "lse", what)
            assert bool((got["nll"] >= 0).all()) and float(got["nll"].max()) < 1e-6 and not bool(torch.isnan(got["dlogits"]).any())
        else:
            judge_all(got, r64, e_ref, False, what)
            assert bool((got["nll"] > 30).all())


# ---- 4. labels that do not count ---------------------------------------------------------------------------------------------
def test_ignored_labels(pkg):
    B, T, V = 3, 9, 257
    logits, labels = make_logits("randn_x3", B, T, V, seed=5), make_labels(B, T, V, seed=5)
    labels[0, 3] = labels[2, 8] = labels[2, 1] = -100
    labels[1, :] = -100                                                         # a whole sequence
    for shift in (True, False):
        r64, e_ref = yardstick(logits, labels, shift=shift)
        got = cabi(pkg, logits, labels, shift=shift)
        judge_all(got, r64, e_ref, shift, f"ignored rows shift={int(shift)}")
        skipped = (labels[:, 1:] if shift else labels) == -100
        assert got["count"] == int((~skipped).sum())
        assert not bool(scored(got, shift).cpu()[skipped].any()) and not bool(got["dlogits"].cpu()[:, :T - int(shift)][skipped].any())
    other = cabi(pkg, logits, labels, ignore_index=int(labels[0, 1]))           # another ignore_index: -100 is then out of range
    assert other["count"] > 0 and float(other["nll"][0, 0]) == 0.0 and not bool(other["dlogits"][0, 0].any())


@pytest.mark.parametrize("B,T,shift", [(2, 9, True), (2, 9, False), (3, 1, True)])
def test_no_row_counts(pkg, B, T, shift):
    """Every label ignored, and T = 1 under the shift: mean NaN, sum 0, count 0, gradient exact zeros under each reduction."""
    V = 65
    logits = make_logits("randn", B, T, V, seed=6)
    labels = torch.full((B, T), -100, dtype=torch.int64) if T > 1 else make_labels(B, T, V, seed=6)
    for reduction in ("mean", "sum", "none"):
        got = cabi(pkg, logits, labels, shift=shift, reduction=reduction)
        assert got["count"] == 0 and float(got["sum"]) == 0.0 and bool(torch.isnan(got["mean"]))
        assert not bool(got["nll"].any()) and not bool(got["dlogits"].any()) and not bool(torch.isnan(got["lse"]).any())
    x = logits.to(DEV).requires_grad_(True)
    loss = pkg.lm_cross_entropy(x, labels.to(DEV), shift=shift)
    loss.backward()
    assert bool(torch.isnan(loss)) and not bool(x.grad.any())
    none = pkg.lm_cross_entropy(x, labels.to(DEV), shift=shift, reduction="none")
    assert none.shape == (B, T - int(shift))
    none.sum().backward()                                                       # an empty upstream gradient at T = 1
    assert not bool(x.grad.any())


def test_out_of_range_label_poisons_its_row_only(pkg):
    B, T, V = 2, 9, 257
    logits, labels = make_logits("randn", B, T, V, seed=7), make_labels(B, T, V, seed=7)
    want = cabi(pkg, logits, labels, reduction="sum")
    for bad in (V, -5, 1 << 40):
        lab = labels.clone()
        lab[1, 4] = bad                                                         # scores row (1, 3)
        got = cabi(pkg, logits, lab, reduction="sum")
        keep = torch.ones(B, T, dtype=torch.bool)
        keep[1, 3] = False
        assert bool(torch.isnan(got["nll"][1, 3])) and bool(torch.isnan(got["dlogits"][1, 3]).all())
        assert torch.equal(got["nll"].cpu()[keep], want["nll"].cpu()[keep])
        assert torch.equal(got["dlogits"].cpu()[keep], want["dlogits"].cpu()[keep]) and torch.equal(got["lse"], want["lse"])
        assert bool(torch.isnan(got["sum"])) and got["count"] == want["count"]
    again = cabi(pkg, logits, labels, reduction="sum")                          # the process is healthy
    assert torch.equal(again["dlogits"], want["dlogits"]) and torch.equal(again["sum"], want["sum"])


def test_minus_infinity_entries_have_probability_zero(pkg):
    B, T, V = 2, 9, 1029
    logits, labels = make_logits("randn_x3", B, T, V, seed=8), make_labels(B, T, V, seed=8)
    labels[0, 3] = labels[1, 6] = 5                                             # no label on a -inf entry
    logits[0, 2, 77] = logits[1, 5, 0] = logits[1, 5, V - 1] = float("-inf")
    logits[1, 7, :1024] = float("-inf")                                         # whole chunks, whole threads: only the tail is finite
    labels[1, 8] = V - 2
    r64, e_ref = yardstick(logits, labels)
    got = cabi(pkg, logits, labels)
    judge_all(got, r64, e_ref, True, "-inf entries")
    assert not bool(got["dlogits"].cpu()[torch.isinf(logits)].any())


# ---- 5. reductions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["sum", "none", "mean"])
def test_reductions_and_upstream_gradients(pkg, reduction):
    B, T, V = 2, 9, 4099
    logits, labels = make_logits("randn_x3", B, T, V, seed=9), make_labels(B, T, V, seed=9)
    labels[1, 2] = -100
    gen = torch.Generator().manual_seed(10)
    upstream = {"sum": torch.tensor(1.0), "none": torch.randn(B, T - 1, generator=gen), "mean": torch.tensor(0.37)}[reduction]
    r64, e_ref = yardstick(logits, labels, reduction=reduction, upstream=upstream)
    judge_all(cabi(pkg, logits, labels, reduction=reduction, upstream=upstream), r64, e_ref, True, f"reduction={reduction}")
    x = logits.to(DEV).requires_grad_(True)
    out = pkg.lm_cross_entropy(x, labels.to(DEV), reduction=reduction)
    assert out.shape == r64["out"].shape and bar_ratio(out, r64["out"]) <= 1.0 + max(e_ref["nll"], e_ref["sum"], e_ref["mean"])
    out.backward(upstream.to(DEV))
    judge(x.grad, r64, e_ref, "dlogits", f"lm_cross_entropy reduction={reduction}")


def test_rows_by_vocabulary_input(pkg):
    """[rows, V] logits with [rows] labels, shift off: the reference's flattened call."""
    logits, labels, r64, e_ref = cached_case("randn", 1, 9, 257, False, 12)
    x = logits[0].to(DEV).requires_grad_(True)
    out = pkg.lm_cross_entropy(x, labels[0].to(DEV), shift=False, reduction="none")
    assert out.shape == (9,)
    judge(out[None], r64, e_ref, "nll", "[rows, V]")
    pkg.lm_cross_entropy(x, labels[0].to(DEV), shift=False).backward()
    judge(x.grad[None], r64, e_ref, "dlogits", "[rows, V]")


# ---- 6. determinism and independence -----------------------------------------------------------------------------------------
def test_deterministic_and_rows_are_independent(pkg):
    B, T, V = 4, 9, 4101
    logits, labels = make_logits("randn_x3", B, T, V, seed=13), make_labels(B, T, V, seed=13)
    a, b = (cabi(pkg, logits, labels, reduction="sum") for _ in range(2))
    for key in ("nll", "lse", "lse_lo", "sum", "mean", "dlogits"):
        assert torch.equal(a[key], b[key]), key
    halves = [cabi(pkg, logits[i:i + 2], labels[i:i + 2], reduction="sum") for i in (0, 2)]
    for key in ("nll", "lse", "lse_lo", "dlogits"):
        assert torch.equal(a[key], torch.cat([h[key] for h in halves])), key
    poisoned = logits.clone()
    poisoned[2, 4, 1000] = NAN
    c = cabi(pkg, poisoned, labels, reduction="sum")
    keep = torch.ones(B, T, dtype=torch.bool)
    keep[2, 4] = False
    assert bool(torch.isnan(c["nll"][2, 4])) and bool(torch.isnan(c["dlogits"][2, 4]).all())
    assert torch.equal(c["nll"].cpu()[keep], a["nll"].cpu()[keep]) and torch.equal(c["dlogits"].cpu()[keep], a["dlogits"].cpu()[keep])


# ---- 7. the Python path ------------------------------------------------------------------------------------------------------
def _launched(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def _has(names, kernel):
    return any(kernel in n for n in names)


def test_autograd_function_and_token_nll(pkg):
    logits, labels, r64, e_ref = cached_case("randn_x3", 2, 9, 4099, True, 4099)
    want = cabi(pkg, logits, labels)
    x, lab = logits.to(DEV).requires_grad_(True), labels.to(DEV)
    loss = pkg.lm_cross_entropy(x, lab)
    saved = loss.grad_fn.saved_tensors
    assert sum(t.numel() for t in saved if t.data_ptr() != x.data_ptr()) <= 3 * lab.numel() + 1   # labels, the lse pair, the count
    loss.backward()
    assert torch.equal(loss, want["mean"]) and torch.equal(x.grad, want["dlogits"])
    with pytest.raises(RuntimeError):
        (g,) = torch.autograd.grad(pkg.lm_cross_entropy(x, lab), x, create_graph=True)
        g.sum().backward()
    none = pkg.lm_cross_entropy(x, lab, reduction="none")
    nll = pkg.token_nll(x, lab)
    assert nll.shape == (2, 8) and not nll.requires_grad and torch.equal(nll, none.detach()) and torch.equal(nll, scored(want, True))
    # no backward launch for logits that need no gradient, none at all with gradients disabled
    w = torch.ones((), device=DEV, requires_grad=True)
    names = _launched(lambda: (pkg.lm_cross_entropy(x.detach(), lab) * w).backward())
    assert _has(names, KERNELS[0]) and _has(names, KERNELS[1]) and not _has(names, KERNELS[2])
    with torch.no_grad():
        assert pkg.lm_cross_entropy(x, lab).grad_fn is None
    for bad_x, bad_l in ((x.half(), lab), (x, lab.int()), (x.transpose(0, 1), lab.t()), (x[:, :, :0], lab), (x, lab[:, :4])):
        assert not pkg.lm_loss.served(bad_x, bad_l)
        with pytest.raises((ValueError, TypeError)):
            pkg.lm_cross_entropy(bad_x, bad_l)
    assert pkg.lm_loss.served(x, lab)


def test_stream_capture_replays(pkg):
    V = 4099
    logits, labels = make_logits("randn_x3", 2, 9, V, seed=14), make_labels(2, 9, V, seed=14)
    want = cabi(pkg, logits, labels)
    x, lab = logits.to(DEV).requires_grad_(True), labels.to(DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                               # warm-up on the capture stream
        torch.autograd.grad(pkg.lm_cross_entropy(x, lab), x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                                  # one stream, no parallel branches
        loss = pkg.lm_cross_entropy(x, lab)
        (grad,) = torch.autograd.grad(loss, x)
    for _ in range(2):
        grad.fill_(NAN)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(grad, want["dlogits"]) and torch.equal(loss, want["mean"])
    new_logits, new_labels = make_logits("randn", 2, 9, V, seed=15), make_labels(2, 9, V, seed=15)
    with torch.no_grad():
        x.copy_(new_logits)                                                     # new contents, same addresses
    lab.copy_(new_labels)
    graph.replay()
    torch.cuda.synchronize()
    new = cabi(pkg, new_logits, new_labels)
    assert torch.equal(grad, new["dlogits"]) and torch.equal(loss, new["mean"])


# ---- 8. the module -----------------------------------------------------------------------------------------------------------
def test_lm_head_model_at_32_bits(pkg):
    """No quantizer at 32 bits, so no level can flip: the loss and every parameter gradient are judged against a float64 CPU copy of
    the model, with e_ref the torch-path run's own err/bound.  The flag moves the loss onto the new kernels and off log_softmax /
    nll_loss; off, the step is the parent's: same kernels, same bits."""
    cfg = types.SimpleNamespace(vocab_size=131, n_positions=16, n_embd=64, n_layer=2, n_head=2, layer_norm_epsilon=1e-5,
                                embd_pdrop=0.0, bit_widths=[4, 32], lora_rank_per_bit={4: 4, 32: 0}, lora_alpha_per_bit={4: 8, 32: 0},
                                quantizer_per_bit={4: "minmax", 32: None}, per_channel_quantization=True)
    torch.manual_seed(0)
    model = pkg.SPLMHeadModel(cfg)
    model.set_precision(32)
    model.train()
    assert model.use_hip_loss is False
    ids = torch.randint(cfg.vocab_size, (2, 16), generator=torch.Generator().manual_seed(1))
    ref = copy.deepcopy(model).double()
    pkg.set_attention_core(ref, "explicit")
    out64 = ref(ids, labels=ids)
    out64["loss"].backward()
    want = {n: p.grad for n, p in ref.named_parameters() if p.grad is not None}
    model = model.to(DEV)

    def step(loss_path):
        assert pkg.set_lm_loss(model, loss_path) == 1
        model.zero_grad(set_to_none=True)
        box = {}

        def run():
            box["out"] = model(ids.to(DEV), labels=ids.to(DEV))
            box["out"]["loss"].backward()
        names = _launched(run)
        return names, box["out"], {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    step("torch")                                                               # one-time launches stay out of the traces
    names_t, out_t, g_t = step("torch")
    names_h, out_h, g_h = step("hip")
    names_t2, out_t2, g_t2 = step("torch")
    assert all(_has(names_h, k) for k in KERNELS), names_h
    norm = lambda n: n.lower().replace("_", "")
    torch_only = {n for n in names_t if n not in set(names_h)}                  # what the torch loss launches and the HIP step does not
    print(f"[lm loss] kernels of the torch loss only: {sorted(torch_only)}")
    assert any("nllloss" in norm(n) for n in torch_only) and any("softmax" in norm(n) for n in torch_only), torch_only
    assert not any("nllloss" in norm(n) or "logsoftmax" in norm(n) for n in names_h), names_h
    assert not any(_has(names_t, k) for k in KERNELS) and sorted(names_t) == sorted(names_t2)
    assert torch.equal(out_t["loss"], out_t2["loss"]) and all(torch.equal(g_t[n], g_t2[n]) for n in g_t)
    assert torch.equal(out_h["logits"], out_t["logits"]) and out_h["logits"].shape == (2, 16, 131)
    assert set(g_h) == set(g_t) == set(want) and len(want) > 8
    e_loss = bar_ratio(out_t["loss"], out64["loss"])
    r_loss = bar_ratio(out_h["loss"], out64["loss"])
    print(f"[lm loss] SPLMHeadModel loss: err/bound {r_loss:.3f} (torch path {e_loss:.3f})")
    assert r_loss <= 1.0 + e_loss
    for n in want:
        e, r = bar_ratio(g_t[n], want[n]), bar_ratio(g_h[n], want[n])
        print(f"[lm loss] SPLMHeadModel {n}: err/bound {r:.3f} (torch path {e:.3f})")
        assert r <= 1.0 + e, (n, r, e)
