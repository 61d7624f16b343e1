"""Batch-size invariance of the fused forward at every launch choice that depends on M, the token count.

spq_linear_lora_fwd picks, from M alone: 16- or 32-row streaming activation workgroups ((M + 31) / 32 >= CUs), the panel kernel's
chunk count (ceil(M / 32) >= 2 CUs), the persistent grids of the contraction kernels and the split-K factor S (both from the tile
count).  None of them may change a row's bits, except S: the per-tile k split depends on S (and the stage count) only, so a row
sees the same fp32 sums wherever S agrees.  Every case below runs one calibrated layer on M_big = 64 CUs + 37 rows and on three row
slices of the same input (the first 100 rows, 4100 rows from row 4000, the last 77), and compares the slices with the same rows
of the big run:
  * SPQ_SPLIT_K=0: bit-identical;
  * default switches: bit-identical where the library's S (spq_debug_split_k) agrees for the two M; where it does not, within
    5e-6 of the big run (fp32 re-association, as tests/test_gpu_splitk.py) and within the oracle bound where an oracle is given.
Before every call the layer's scratch (the stream's workspace, and the level-matrix slot for the CPT pair) is filled with 0xFF
bytes, which read as NaN in fp32 and fp16: a padded row or column that reached a stored row, or a split-K counter the library did
not zero, would show up as NaN or as a changed row.  Each case asserts that M_big and the small slices fall on opposite sides of
the threshold it is named after."""
import os

import pytest
import torch
import torch.nn.functional as F

from helpers import assert_close_y, oracle_layer_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLICES = ((0, 100), (4000, 8100), (-77, None))


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    return p


@pytest.fixture(autouse=True)
def _restore(pkg):
    old = os.environ.get("SPQ_SPLIT_K")
    yield
    pkg._lib.set_switch("SPQ_SPLIT_K", old)


def cus():
    """the CU count the library sizes its grids by (gemm_grid: a multiple of 8)"""
    return torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8


def m_big():
    return 64 * cus() + 37


def pad(v, m):
    return (v + m - 1) // m * m


# the M-dependent decisions of spq_f16x2.hip, as functions of M (True: the large-M side)
def rows32(M, K, N):                  # 32-row streaming workgroups
    return (M + 31) // 32 >= cus()


def panel_small(M, K, N):             # xpass_panel_kernel<XP_CHUNKS_SMALL>
    return (M + 31) // 32 >= 2 * cus()


def t128_tiles(M, K, N):              # 128 x 128 tiles fill the t128 kernel's slots: no split-K, a persistent grid
    return (pad(M, 256) // 128) * (pad(N, 128) // 128) >= 3 * cus()


def i8_k128_grid(M, K, N):            # gemm_i8_k128_kernel: persistent grid of 2 CUs
    return 2 * (pad(M, 256) // 256) * (pad(N, 128) // 128) >= 2 * cus()


def i8_ring_grid(M, K, N):            # gemm_i8_kernel: one workgroup per CU
    return (pad(M, 256) // 256) * (pad(N, 128) // 128) >= cus()


def slices_of(M):
    return [(a, b if b is not None else M) if a >= 0 else (M + a, M) for a, b in SLICES]


def assert_crosses(decisions, K, N):
    """every named decision is taken one way at M_big and the other way for the 100- and 77-row slices (the 4100-row slice also
    crosses the row-count thresholds)"""
    Mb = m_big()
    for d in decisions:
        for a, b in slices_of(Mb):
            if b - a < 4100 or d in (rows32, panel_small):
                assert d(Mb, K, N) != d(b - a, K, N), (d.__name__, Mb, b - a)


def fill_scratch(pkg, nbytes, slots=(0,)):
    for s in slots:
        pkg._lib.workspace(torch.device(DEV), nbytes, slot=s).fill_(0xFF)


def predicted_split(pkg, M, K, N, r, path, no_split=False):
    """The forward's S.  It never splits with a GELU or levels-out epilogue or on the int8 path (spq_f16x2.hip fwd_f16x2), and it
    counts LoRA stages only when the LoRA-up operand is there: r is 0 for LoRA-down-only and contraction-only calls."""
    if no_split or path not in (pkg._lib.PATH_F16X2, pkg._lib.PATH_F16X3):
        return 1
    return int(pkg._lib.load().spq_debug_split_k(M, K, N, r, path))


def check_slices(pkg, run, X, split_of, nbytes, slots=(0,), oracle=None, must_differ=False):
    """run(x) -> output rows of x.  split_of(M) -> the S the library takes for M rows.  Returns how many slices had another S."""
    Mb = X.shape[0]
    n_differ = 0
    for mode in ("0", None):
        pkg._lib.set_switch("SPQ_SPLIT_K", mode)
        fill_scratch(pkg, nbytes, slots)
        with torch.no_grad():
            big = run(X).clone()
        assert bool(torch.isfinite(big).all()), f"SPQ_SPLIT_K={mode}: non-finite output at M={Mb}"
        fill_scratch(pkg, nbytes, slots)
        with torch.no_grad():
            assert torch.equal(run(X), big), f"SPQ_SPLIT_K={mode}: M={Mb} not bit-identical run to run"
        for a, b in slices_of(Mb):
            fill_scratch(pkg, nbytes, slots)
            with torch.no_grad():
                y = run(X[a:b].contiguous())
            assert bool(torch.isfinite(y).all()), f"SPQ_SPLIT_K={mode}: non-finite output in rows {a}:{b} run alone"
            s_big, s_small = (1, 1) if mode == "0" else (split_of(Mb), split_of(b - a))
            what = f"SPQ_SPLIT_K={mode}, rows {a}:{b} (S {s_small}) vs the same rows of M={Mb} (S {s_big})"
            if s_big == s_small:
                assert torch.equal(y, big[a:b]), f"{what}: {int((y != big[a:b]).any(dim=-1).sum())} rows differ"
            else:
                n_differ += 1
                assert_close_y(y, big[a:b], what, 5e-6)
                if oracle is not None:
                    ref = oracle(X[a:b])
                    assert_close_y(y, ref, what + " vs oracle", 1e-5)
                    assert_close_y(big[a:b], ref, f"rows {a}:{b} of M={Mb} vs oracle", 1e-5)
    if must_differ:
        assert n_differ > 0, "the split-K factor never differs between the two batch sizes: the comparison above is vacuous"
    return n_differ


def activations(M, K, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x = torch.where(torch.rand(M, K, generator=g) < 1e-3, x * 20, x)
    return (x * scale + shift).to(DEV)


def sp_layer(pkg, K, N, r, bits, qtype, per_channel=True, seed=0, ln=None):
    from llm_qat_on_gpt2_amd import synthetic as S
    W, bias, A, B, _, _ = S.make_workload(8, K, N, max(r, 1), seed=seed)
    layer = pkg.SPLinearWithLoRA(K, N, [bits, 32], {bits: r, 32: 0}, {bits: max(r, 1), 32: 0}, {bits: qtype, 32: None},
                                 per_channel=per_channel)
    key = f"{bits}bit"
    with torch.no_grad():
        layer.linear.weight.copy_(W); layer.linear.bias.copy_(bias)
        if r:
            layer.lora_adapters[key].lora_A.copy_(A); layer.lora_adapters[key].lora_B.copy_(B)
    layer = layer.to(DEV).eval()
    layer.set_precision(bits)
    cal = [activations(2048, K, seed + 1 + i) for i in range(2)]
    with torch.no_grad():
        pkg.calibrate_layer(layer, bits, [ln(c) for c in cal] if ln is not None else cal)
    return layer


def layernorm(pkg, K, bits):
    ln = pkg.SwitchableLayerNorm(K, precision_levels=[bits, 32], eps=1e-5)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        ln.weights[str(bits)].copy_(torch.randn(K, generator=g) * 0.2 + 1.0); ln.biases[str(bits)].copy_(torch.randn(K, generator=g) * 0.1)
    ln = ln.to(DEV)
    ln.set_precision(bits)
    return ln


def ws_bytes(pkg, M, K, N, r=128):
    lib = pkg._lib.load()
    return max(lib.spq_fwd_workspace_bytes(M, K, N, r, p) for p in (pkg._lib.PATH_F16X2, pkg._lib.PATH_F16X3, pkg._lib.PATH_I8)) \
        + pkg._lib.LIMB_SCALE_WORKSPACE_BYTES + 4096


def sp_oracle(layer, bits, ln=None):
    from oracle import ref_cpu as O
    ol = oracle_layer_of(layer, bits)
    if ln is None:
        return lambda x: ol.forward(x.cpu())
    w, b = ln.weights[str(bits)].detach().cpu(), ln.biases[str(bits)].detach().cpu()
    return lambda x: ol.forward(O.switchable_layernorm(x.cpu(), w, b, float(ln.eps)))


# ---------------------------------------------------------------------------------------------------------------------------
# SPLinearWithLoRA on the F16X2 / F16X3 / I8 paths
# (name, K, N, r, bits, qtype, per_channel, variant, path, decisions crossed, the split-K factor must differ)
#   variant: plain | ln (LayerNorm prologue) | gelu | prep (role-fused weight rows) | calib (no LoRA term) | f32 (PATH_F32 forced)
SP_CASES = [
    ("f16x2", 768, 3072, 64, 4, "minmax", True, "plain", 2, (rows32, t128_tiles), False),
    ("f16x2_ln", 768, 3072, 64, 4, "minmax", True, "ln", 2, (rows32, t128_tiles), False),
    ("f16x2_gelu", 768, 3072, 64, 4, "minmax", True, "gelu", 2, (rows32, t128_tiles), False),
    ("f16x2_role_prep", 768, 3072, 64, 4, "minmax", True, "prep", 2, (rows32, t128_tiles), False),
    ("f16x3_log", 1024, 1024, 64, 6, "log", True, "plain", 4, (rows32, t128_tiles), True),
    ("f16x3_log_ln", 1024, 1024, 64, 6, "log", True, "ln", 4, (rows32, t128_tiles), True),
    ("i8_k128", 768, 3072, 64, 8, "minmax", False, "plain", 5, (rows32, i8_k128_grid), False),
    ("i8_ring", 320, 1024, 64, 8, "minmax", False, "plain", 5, (rows32, i8_ring_grid), False),
    ("f16x2_mlp_c_proj", 3072, 768, 64, 4, "minmax", True, "plain", 2, (rows32, t128_tiles), True),
    ("f16x2_no_lora", 768, 3072, 64, 4, "minmax", True, "calib", 2, (panel_small, t128_tiles), False),
    ("f32", 768, 1024, 64, 4, "minmax", True, "f32", 1, (), False),      # gemm_f32_nt: one workgroup per tile, no M-dependent choice
]


@pytest.mark.parametrize("case", SP_CASES, ids=lambda c: c[0])
def test_layer_rows_do_not_depend_on_the_batch(pkg, case):
    name, K, N, r, bits, qtype, pc, variant, path, decisions, must_differ = case
    assert_crosses(decisions, K, N)
    ln = layernorm(pkg, K, bits) if variant == "ln" else None
    layer = sp_layer(pkg, K, N, r, bits, qtype, per_channel=pc, seed=K + N + bits, ln=ln)
    if variant == "calib":
        layer.calibration_mode = True
    if variant == "prep":
        layer.cache_operands = False                       # every forward re-quantises: the weight rows ride in the activation launch
        assert layer.fuse_prepare
    if variant == "f32":
        layer.operand_path = pkg._lib.PATH_F32
    X = activations(m_big(), K, seed=7 + K, scale=1.7 if ln else 1.0, shift=0.3 if ln else 0.0)
    if ln is not None:
        X[:, 3] += 25.0                                    # an outlier channel, as GPT-2 residual streams have

    def run(x):
        y = layer(x, activation="gelu" if variant == "gelu" else None, pre_norm=ln)
        assert layer._last_path == path, (layer._last_path, path)
        assert layer._norm_fused == (ln is not None)
        return y

    use_r = 0 if variant == "calib" else r
    split_of = lambda M: predicted_split(pkg, M, K, N, use_r, path, no_split=variant == "gelu")
    oracle = sp_oracle(layer, bits, ln) if qtype == "minmax" and variant in ("plain", "ln") else None
    check_slices(pkg, run, X, split_of, ws_bytes(pkg, m_big(), K, N), oracle=oracle, must_differ=must_differ)


# ---------------------------------------------------------------------------------------------------------------------------
# part2: CPTLinear (panel kernel, LoRA read from FQ(x) and folded into the weight) and the levels-out pair cpt_mlp_forward
def test_cpt_rows_do_not_depend_on_the_batch(pkg):
    from test_gpu_cpt_mlp import make_chain
    E, H, bits = 768, 3072, 4
    fc_in, fc_out, _, _, _ = make_chain(pkg, E, H, bits, "minmax", 1024, seed=11)
    assert_crosses((panel_small, t128_tiles), E, H)
    assert_crosses((panel_small, t128_tiles), H, E)
    X = activations(m_big(), E, seed=12)
    lib = pkg._lib.load()
    nbytes = ws_bytes(pkg, m_big(), H, H)
    assert lib.spq_fwd_workspace_bytes(m_big(), H, E, 0, pkg._lib.PATH_F16X3) <= nbytes

    from llm_qat_on_gpt2_amd.cpt import _QuantGemm
    p_in, p_out = (_QuantGemm.path_for(m.quantizer_input, m.out_features, True) for m in (fc_in, fc_out))
    assert pkg._lib.PATH_F32 not in (p_in, p_out)

    def run_in(x):
        y = fc_in(x)
        assert fc_in._last_path == p_in
        return y
    check_slices(pkg, run_in, X, lambda M: predicted_split(pkg, M, E, H, 0, p_in), nbytes)

    def run_pair(x):
        return pkg.cpt_mlp_forward(fc_in, fc_out, x)
    with torch.no_grad():
        xs = X[:512]
        assert torch.equal(run_pair(xs), fc_out(F.gelu(fc_in(xs)))), "cpt_mlp_forward differs from its two-layer form"
    # the producer (GELU + levels-out store) never splits; the consumer is contraction-only, with no LoRA stages
    check_slices(pkg, run_pair, X, lambda M: predicted_split(pkg, M, H, E, 0, p_out), nbytes, slots=(0, 1),
                 must_differ=True)


# ---------------------------------------------------------------------------------------------------------------------------
# the backward's g . FQ(W) (sp_linear._LimbGemm): the gradient operand's limb scale 2^G comes from max|g| over the whole batch
@pytest.mark.parametrize("with_down", [False, True], ids=["gx", "gx_and_down"])
def test_backward_limb_gemm_rows_do_not_depend_on_the_batch(pkg, with_down):
    """_LimbGemm splits the gradient into two fp16 limbs of g * 2^G, with max|g| * 2^G in [2^13, 2^14) over the WHOLE batch, so
    a row's G changes with the rows around it.  Its bits do not, as long as the limbs of each element are exact multiples of
    the same limbs at another G: 2^G is a power of two and, when every nonzero element has |g| * 2^G >= 1 at the smaller G,
    both fp16 limbs stay normal (or the low limb is exact), the fp16 products are exact in fp32 and the fp32 sums scale with
    2^G.  Here every element lies within 2^-4 of its row's maximum and every row within 2^-1 of every other, and one batch
    also holds a row 2^8 times larger (G lower by 8): the rows must come out bit for bit as they do alone.  (The accuracy of
    rows far smaller than the batch maximum, where the low limb goes subnormal, is a separate matter: per-row limb scales.)"""
    from llm_qat_on_gpt2_amd import sp_linear as SL
    C, R, r = 3072, 768, 64                               # gx of mlp.c_fc: g [M, 4E] . FQ(W) [4E, E]
    Mb = m_big()
    assert_crosses((panel_small, t128_tiles), C, R)
    g = torch.Generator().manual_seed(21)
    b = (torch.randn(R, C, generator=g) * 0.02).to(DEV)
    down = (torch.randn(r, C, generator=g) * 0.01).to(DEV) if with_down else None
    mag = 2.0 ** (-4 * torch.rand(Mb, C, generator=g)) * (1 - 0.5 * torch.rand(Mb, 1, generator=g))
    G = (torch.where(torch.rand(Mb, C, generator=g) < 0.5, -mag, mag) * 1.5e-3).to(DEV)
    gm = SL._LimbGemm()
    lib = pkg._lib.load()
    nbytes = lib.spq_fwd_workspace_bytes(Mb, C, R, r, pkg._lib.PATH_F16X3) + pkg._lib.LIMB_SCALE_WORKSPACE_BYTES + 4096
    scales = {}

    def run(x):
        out = gm(x, b, down)
        scales[x.shape[0]] = float(gm.xscale[0])
        return out if down is None else torch.cat(out, dim=1)   # [gx | g . down^T]
    split_of = lambda M: predicted_split(pkg, M, C, R, 0, pkg._lib.PATH_F16X3)   # LoRA-down only: no LoRA stages
    ref = lambda x: torch.cat([x.double() @ b.double().t()] + ([x.double() @ down.double().t()] if with_down else []), dim=1).float()
    check_slices(pkg, run, G, split_of, nbytes, oracle=ref, must_differ=True)
    # one row 2^8 times larger (outside the slices): the batch's G drops by 8, the slices keep theirs
    G[2000] *= 256.0
    check_slices(pkg, run, G, split_of, nbytes, oracle=ref, must_differ=True)
    assert scales[100] >= 128.0 * scales[Mb], (scales[Mb], scales[100])           # the big batch really ran at another G
