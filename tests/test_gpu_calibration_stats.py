"""Calibration statistics (spq_minmax_stats, spq_dynamic_limb_scale) with PLANTED extrema at every launch edge.

min / max reductions hide a skipped element unless the extremum lies exactly there, so random data cannot test the loop bounds of
these kernels.  Here the background lies inside a band and each channel's minimum and maximum are planted outside it, at
positions that sweep every row, column, chunk border and loop tail of each dispatch path (planners and their coverage claims:
tests/stats_ref.py, proved by counting in tests/test_stats_ref_cpu.py).  All planted values are powers of two, so every
comparison -- linear and log domain -- is torch.equal against stats_ref.expected, with no element excluded.

A sweep stays on the device: plant with an in-place write, launch, restore, with min_io / max_io pointing at row p of one result
matrix; one synchronisation and one comparison at the end.
"""
import math

import numpy as np
import pytest
import torch

import stats_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = R.EPS_LOG
FILL = -17.0                    # fp32 log2(EPS)
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    return p


def _workspace(lib, outer, chan, inner, per_channel):
    need = lib.spq_stats_workspace_bytes(outer, chan, inner, int(per_channel))
    assert need > 0
    return torch.empty(need, dtype=torch.uint8, device=DEV)


def _stats(pkg, x, outer, chan, inner, per_channel, log, first, lo, hi, ws=None):
    """One spq_minmax_stats call on device tensors; lo / hi are updated in place."""
    lib = pkg._lib.load()
    assert x.numel() == outer * chan * inner and lo.numel() == hi.numel() == (chan if per_channel else 1)
    ws = _workspace(lib, outer, chan, inner, per_channel) if ws is None else ws
    rc = lib.spq_minmax_stats(x.data_ptr(), outer, chan, inner, int(per_channel), int(log), EPS, FILL, int(first),
                              lo.data_ptr(), hi.data_ptr(), ws.data_ptr(), ws.numel(), pkg._lib.stream_ptr(torch.device(DEV)))
    pkg._lib.check(rc, "spq_minmax_stats")


def _device_copy(flat, offset):
    """`flat` on the device, `offset` floats behind a 16-byte aligned address."""
    buf = torch.empty(flat.numel() + offset, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    x = buf[offset:]
    x.copy_(flat)
    return x


def _sweep(pkg, pr, offset=0, prev=None):
    """Every variant of `pr` through spq_minmax_stats.  prev=None: first batch; else (lo, hi) scalars the outputs are prefilled
    with before a later-batch call.  Returns (min [P, C], max [P, C]) on the CPU."""
    lib = pkg._lib.load()
    P, C = pr.idx.shape[0], (pr.chan if pr.per_channel else 1)
    x = _device_copy(pr.bg, offset)
    idx, vals = pr.idx.to(DEV), pr.vals.to(DEV)
    saved = x[idx]
    out = torch.full((2, P, C), SENTINEL, dtype=torch.float32, device=DEV)
    if prev is not None:
        out[0].fill_(prev[0]); out[1].fill_(prev[1])
    ws = _workspace(lib, pr.outer, pr.chan, pr.inner, pr.per_channel)
    idx_rows, val_rows, saved_rows = idx.unbind(0), vals.unbind(0), saved.unbind(0)
    xp, wp, wn = x.data_ptr(), ws.data_ptr(), ws.numel()
    lo_p, hi_p = out[0].data_ptr(), out[1].data_ptr()
    stream = pkg._lib.stream_ptr(torch.device(DEV))
    pc, lg, first = int(pr.per_channel), int(pr.log), int(prev is None)
    for p in range(P):
        x.index_copy_(0, idx_rows[p], val_rows[p])
        rc = lib.spq_minmax_stats(xp, pr.outer, pr.chan, pr.inner, pc, lg, EPS, FILL, first, lo_p + 4 * C * p, hi_p + 4 * C * p,
                                  wp, wn, stream)
        if rc:
            pkg._lib.check(rc, "spq_minmax_stats")
        x.index_copy_(0, idx_rows[p], saved_rows[p])
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), pr.bg), "the sweep did not restore its background"
    return out[0].cpu(), out[1].cpu()


def _check_sweep(pkg, pr, what, offset=0):
    lo, hi = _sweep(pkg, pr, offset)
    e_lo, e_hi = pr.expected()
    for name, got, ref in (("min", lo, e_lo), ("max", hi, e_hi)):
        if not torch.equal(got, ref):
            bad = torch.nonzero(got != ref)
            p, c = bad[0].tolist()
            raise AssertionError(f"{what}: {name} differs in {len(bad)} of {got.numel()} results; first at variant {p} (planted at "
                                 f"{pr.idx[p].tolist()[:4]}...), channel {c}: got {float(got[p, c])!r}, expected {float(ref[p, c])!r}")


# ---- flat path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True])
def test_flat_every_position(pkg, log):
    T = R.FLAT_TOTAL
    _check_sweep(pkg, R.flat_probes(T, range(T), log, 11), f"flat total={T}")


@pytest.mark.parametrize("log", [False, True])
def test_flat_unaligned_pointer(pkg, log):
    T = R.FLAT_TOTAL
    _check_sweep(pkg, R.flat_probes(T, R.thinned(T, 5), log, 15), f"flat total={T} pointer+1", offset=1)


@pytest.mark.parametrize("log", [False, True])
def test_flat_small_totals(pkg, log):
    for total in R.FLAT_SMALL_TOTALS:
        for offset in (0, 1):
            _check_sweep(pkg, R.flat_probes(total, R.thinned(total, 3), log, 12), f"flat total={total} pointer+{offset}", offset)


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("total", R.FLAT_CAPPED_TOTALS)
def test_flat_capped_slab_count(pkg, total, log):
    _check_sweep(pkg, R.flat_probes(total, R.flat_capped_positions(total, 13), log, 14), f"flat total={total}")


# ---- column path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("cols", R.COLS_COLS)
def test_cols_every_row_every_column(pkg, cols, log):
    for rows in R.COLS_ROWS:
        _check_sweep(pkg, R.cols_probes(rows, cols, log, 21), f"cols rows={rows} cols={cols}")


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("cols", [68, 5])
def test_cols_slab_count_sweep(pkg, cols, log):
    """rows = 16 * S: S slabs of 16 rows into the merge kernel (its stride-4 and stride-8 loops and their tails)."""
    for rows in R.COLS_SLAB_SWEEP:
        _check_sweep(pkg, R.cols_probes(rows, cols, log, 22), f"cols rows={rows} cols={cols}")


@pytest.mark.parametrize("log", [False, True])
def test_cols_unaligned_pointer(pkg, log):
    _check_sweep(pkg, R.cols_probes(33, 260, log, 23), "cols rows=33 cols=260 pointer+1", offset=1)


# ---- row path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("chan", R.ROWS_CHAN)
def test_rows_every_position(pkg, chan, log):
    for inner in R.ROWS_INNER:
        L = None if inner <= 257 else R.rows_long_positions(inner, 31)
        _check_sweep(pkg, R.rows_probes(chan, inner, log, 32, L), f"rows chan={chan} inner={inner}")


# ---- two-stage path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("shape", R.TWO_STAGE_SHAPES)
def test_two_stage_planted(pkg, shape, log):
    _check_sweep(pkg, R.two_stage_probes(*shape, log, 41), f"two-stage {shape}")


@pytest.mark.parametrize("qtype", ["minmax", "log"])
@pytest.mark.parametrize("contiguous", [True, False])
def test_two_stage_through_module(pkg, qtype, contiguous):
    """LearnableFakeQuantize(channel_dim=1) on a 4-D tensor [3, 5, 2, 4] -> (outer, chan, inner) = (3, 5, 8); two batches."""
    log = qtype == "log"
    pr = R.two_stage_probes(3, 5, 8, log, 42)
    q = pkg.LearnableFakeQuantize(8, channel_dim=1, quantizer_type=qtype, eps=EPS)
    q.start_calibration()
    prev = None
    for p in (0, 5):
        x = pr.variant(p).reshape(3, 5, 2, 4)
        prev = R.expected(x, 3, 5, 8, True, log, EPS, prev)
        xd = x.to(DEV)
        if not contiguous:
            xd = xd.transpose(1, 3).contiguous().transpose(1, 3)           # same values, another memory order
            assert not xd.is_contiguous() and torch.equal(xd.cpu(), x)
        q(xd)
    q.finish_calibration()
    assert q.running_min.shape == (1, 5, 1, 1)
    assert torch.equal(q.running_min.cpu().reshape(-1), prev[0]) and torch.equal(q.running_max.cpu().reshape(-1), prev[1])


# ---- log domain: the "any element above eps" flag ------------------------------------------------------------------------
def test_log_any_flag_single_element(pkg):
    """2100 x 260: 105 x 260 partial maxima (> 4096).  One element above eps, wherever its partial lands, must switch the update
    on: its channel gets the planted log, every other statistic log2(eps)."""
    pr = R.any_flag_probes(*R.ANY_SHAPE, 51)
    _check_sweep(pkg, pr, "any flag, first batch")
    lo, hi = _sweep(pkg, pr, prev=(5.0, -20.0))                              # a later batch: merged into the running values
    e_lo, e_hi = pr.expected()
    assert torch.equal(lo, torch.clamp(e_lo, max=5.0)) and torch.equal(hi, torch.clamp(e_hi, min=-20.0))
    assert bool((lo == FILL).all()) and int((hi > FILL).sum()) == pr.idx.shape[0]


@pytest.mark.parametrize("view,per_channel", [((2100, 260, 1), True), ((2100, 260, 1), False), ((1, 20, 37), True),
                                              ((5, 20, 7), True), ((3 * 4096 + 5, 1, 1), False)])
def test_log_no_element_above_eps(pkg, view, per_channel):
    x = R.below_eps_background(view, EPS, 52).reshape(-1)
    n_out = view[1] if per_channel else 1
    xd = x.to(DEV)
    lo = torch.full((n_out,), SENTINEL, device=DEV)
    hi = torch.full((n_out,), -SENTINEL, device=DEV)
    _stats(pkg, xd, *view, per_channel, True, False, lo, hi)                # a later batch: bit-untouched
    e_lo, e_hi = R.expected(x, *view, per_channel, True, EPS, prev=(lo.cpu().clone(), hi.cpu().clone()))
    assert torch.equal(lo.cpu().view(torch.int32), e_lo.view(torch.int32)) and torch.equal(hi.cpu().view(torch.int32), e_hi.view(torch.int32))
    assert bool((lo == SENTINEL).all()) and bool((hi == -SENTINEL).all())
    _stats(pkg, xd, *view, per_channel, True, True, lo, hi)                 # a first batch: filled
    e_lo, e_hi = R.expected(x, *view, per_channel, True, EPS)
    assert torch.equal(lo.cpu(), e_lo) and torch.equal(hi.cpu(), e_hi) and bool((lo == FILL).all()) and bool((hi == FILL).all())


@pytest.mark.parametrize("view,per_channel", [((37, 20, 1), False), ((37, 1, 1), True), ((37, 20, 1), True), ((1, 20, 37), True),
                                              ((5, 20, 7), True), ((3 * 4096 + 5, 1, 1), False)])
def test_log_nan_hides_no_element_from_the_eps_test(pkg, view, per_channel):
    """`(|x| > eps).any()` is false for a NaN but true for the element next to it.  A NaN in EVERY partial result (one slab, or
    one in every channel) once made the whole tensor look empty: the NaN vanished into log2(eps) or into the running values."""
    outer, chan, inner = view
    n_out = chan if per_channel else 1
    nan_each = R.background(view, True, 53)
    nan_each[(outer - 1) // 2, :, (inner - 1) // 2] = float("nan")            # a NaN in every channel, ordinary values around it
    if outer > 4096:
        nan_each[::4096] = float("nan")                                       # ... and in every slab of the long flat case
    tiny = R.below_eps_background(view, EPS, 54)
    tiny[0, 0, 0] = float("nan")                                              # a NaN and nothing above eps
    for name, x in (("NaN among ordinary values", nan_each), ("NaN and nothing above eps", tiny), ("only NaN", torch.full(view, float("nan")))):
        for first in (True, False):
            lo = torch.full((n_out,), 3.0, device=DEV)
            hi = torch.full((n_out,), 4.0, device=DEV)
            _stats(pkg, x.reshape(-1).to(DEV), *view, per_channel, True, first, lo, hi)
            e_lo, e_hi = R.expected(x, *view, per_channel, True, EPS, None if first else (torch.full((n_out,), 3.0), torch.full((n_out,), 4.0)))
            for got, ref in ((lo.cpu(), e_lo), (hi.cpu(), e_hi)):
                nan = torch.isnan(ref)
                assert torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], ref[~nan]), (name, first, got, ref)
        if name == "NaN among ordinary values":
            assert bool(torch.isnan(e_lo).all()) and bool(torch.isnan(e_hi).all())
        else:
            assert not bool(torch.isnan(e_lo).any())                          # torch's rule: such a tensor counts as empty


# ---- running merge -------------------------------------------------------------------------------------------------------
def _merge_batches(view, per_channel, log):
    """Three batches: planted extrema everywhere; wider extrema in the even channels only; plain background (narrower)."""
    outer, chan, inner = view
    if not per_channel:
        first = R.flat_probes(outer * chan * inner, [17], log, 61)
    elif inner == 1:
        first = R.cols_probes(outer, chan, log, 61)
    elif outer == 1:
        first = R.rows_probes(chan, inner, log, 61)
    else:
        first = R.two_stage_probes(outer, chan, inner, log, 61)
    b1 = first.variant(0)
    b2 = R.background(view, log, 62)
    for c in range(0, chan, 2):
        sign = -1.0 if log and c % 4 else 1.0                                # the log domain takes |x|: either sign widens
        b2[(c + 1) % outer, c, (2 * c) % inner] = -sign * (2.0 ** -16 if log else 2.0 ** 13)
        b2[c % outer, c, (2 * c + 1) % inner] = sign * 2.0 ** 13
    return [b1, b2.reshape(-1), R.background(view, log, 63).reshape(-1)]


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("view,per_channel", [((37, 20, 1), True), ((1, 20, 37), True), ((5, 20, 7), True), ((37, 20, 1), False)])
def test_running_merge(pkg, view, per_channel, log):
    n_out = view[1] if per_channel else 1
    batches = _merge_batches(view, per_channel, log)
    for poison in (False, True):
        if poison:
            batches[1] = batches[1].clone()
            batches[1].reshape(view)[2 % view[0], 3, 1 % view[2]] = float("nan")
        lo = torch.full((n_out,), SENTINEL, device=DEV)
        hi = torch.full((n_out,), SENTINEL, device=DEV)
        prev, history = None, []
        for n, b in enumerate(batches):
            _stats(pkg, b.to(DEV), *view, per_channel, log, n == 0, lo, hi)
            prev = R.expected(b, *view, per_channel, log, EPS, prev)
            history.append(prev)
            for got, ref in ((lo.cpu(), prev[0]), (hi.cpu(), prev[1])):
                nan = torch.isnan(ref)
                assert torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan], ref[~nan]), (n, poison)
        if poison:                                                           # exactly its channel, and it stays
            want = torch.zeros(n_out, dtype=torch.bool)
            want[3 if per_channel else 0] = True
            for stat in history[1] + history[2]:
                assert torch.equal(torch.isnan(stat), want)
        else:                                                                # the sequence does what its description says
            widened = (history[1][0] < history[0][0]) & (history[1][1] > history[0][1])
            assert widened.tolist() == ([c % 2 == 0 for c in range(n_out)] if per_channel else [True])
            assert torch.equal(history[2][0], history[1][0]) and torch.equal(history[2][1], history[1][1])


# ---- spq_dynamic_limb_scale ----------------------------------------------------------------------------------------------
def _limb_scale(pkg, x, out, ws):
    rc = pkg._lib.load().spq_dynamic_limb_scale(x.data_ptr(), x.numel(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                pkg._lib.stream_ptr(torch.device(DEV)))
    pkg._lib.check(rc, "spq_dynamic_limb_scale")


def _in_guard_band(m):
    """m < 2^k <= fp32(m * (1 + 2^-10)): the scale is chosen for the guarded value, one binade up."""
    m = np.float32(m)
    return math.frexp(float(m))[1] != math.frexp(float(np.float32(m * np.float32(1 + 2.0 ** -10))))[1]


@pytest.mark.parametrize("n", R.LIMB_N)
def test_limb_scale_planted_maximum(pkg, n):
    """out[0] is exactly the header's 2^G, out[1] its reciprocal, and max|x| * 2^G lies in [2^13, 2^14) -- except for a
    maximum inside the 2^-10 guard band below a power of two, where the guarded value m (1 + 2^-10) lies in that interval and
    m * 2^G in [2^13 / (1 + 2^-10), 2^13)."""
    lib = pkg._lib.load()
    pr = R.limb_probes(n, R.limb_positions(n, 71), 72)
    P = pr.idx.shape[0]
    x = pr.bg.to(DEV)
    idx, vals = pr.idx.to(DEV), pr.vals.to(DEV)
    saved = x[idx]
    out = torch.full((P, 2), SENTINEL, dtype=torch.float32, device=DEV)
    ws = torch.empty(pkg._lib.LIMB_SCALE_WORKSPACE_BYTES, dtype=torch.uint8, device=DEV)
    stream = pkg._lib.stream_ptr(torch.device(DEV))
    for p in range(P):
        x.index_copy_(0, idx[p], vals[p])
        rc = lib.spq_dynamic_limb_scale(x.data_ptr(), n, out.data_ptr() + 8 * p, ws.data_ptr(), ws.numel(), stream)
        if rc:
            pkg._lib.check(rc, "spq_dynamic_limb_scale")
        x.index_copy_(0, idx[p], saved[p])
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), pr.bg)
    out = out.cpu()
    # the largest magnitude of every variant, from the reference reduction (not from the plan)
    m_all = R.expected_sweep(pr.bg.abs(), 1, 1, n, False, False, EPS, pr.idx, pr.vals.abs())[1].reshape(-1)
    want = torch.tensor([[float(v) for v in R.limb_scale_expected(float(m))] for m in m_all], dtype=torch.float32)
    assert torch.equal(out, want), f"n={n}: {int((out != want).any(dim=1).sum())} of {P} scales differ"
    assert torch.equal(out[:, 1], 1.0 / out[:, 0])
    scaled = m_all.double() * out[:, 0].double()
    guarded = (m_all * (1 + 2.0 ** -10)).double() * out[:, 0].double()       # the fp32 product the header names
    band = torch.tensor([_in_guard_band(float(m)) for m in m_all])
    assert bool((scaled < 2.0 ** 14).all()) and bool((scaled[~band] >= 2.0 ** 13).all())
    assert bool((guarded >= 2.0 ** 13).all()) and bool((guarded < 2.0 ** 14).all())
    assert P < len(R.LIMB_MAGNITUDES) or int(band.sum()) >= 1


def test_limb_scale_special_inputs(pkg):
    ws = torch.empty(pkg._lib.LIMB_SCALE_WORKSPACE_BYTES, dtype=torch.uint8, device=DEV)
    bg = R.background((3 * 4096 + 5,), True, 73)
    cases = [("zeros", torch.zeros(4101), None, 0.0), ("+inf", bg, float("inf"), float("inf")), ("-inf", bg, float("-inf"), float("inf")),
             ("nan is ignored", torch.cat([bg[:40], 8 * bg[40:41], bg[41:50]]), float("nan"), 8 * float(bg[40].abs())),
             ("tiny", torch.full((5,), 2.0 ** -120), None, 2.0 ** -120), ("scaled down", bg * 2.0 ** -40, None, float(bg.abs().max()) * 2.0 ** -40)]
    for name, x, planted, m in cases:
        x = x.clone()
        if planted is not None:
            x[x.numel() - 2] = planted
        out = torch.full((2,), SENTINEL, device=DEV)
        _limb_scale(pkg, x.to(DEV), out, ws)
        want = tuple(float(v) for v in R.limb_scale_expected(m))
        assert tuple(out.cpu().tolist()) == want, name
        if name in ("zeros", "+inf", "-inf"):
            assert want == (1.0, 1.0)
    assert R.limb_scale_expected(2.0 ** -120)[0] == 2.0 ** 100


# ---- determinism ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log", [False, True])
def test_two_runs_are_bit_identical(pkg, log):
    g = torch.Generator().manual_seed(81)
    for view, per_channel in (((1, 1, 3 * 4096 + 5), False), ((2100, 260, 1), True), ((1, 260, 257), True), ((33, 260, 4), True)):
        x = torch.randn(view, generator=g).reshape(-1).to(DEV)
        n_out = view[1] if per_channel else 1
        runs = []
        for _ in range(2):
            lo = torch.full((n_out,), SENTINEL, device=DEV)
            hi = torch.full((n_out,), SENTINEL, device=DEV)
            _stats(pkg, x, *view, per_channel, log, True, lo, hi)
            runs.append(torch.stack([lo, hi]).cpu().view(torch.int32))
        assert torch.equal(runs[0], runs[1]), (view, per_channel)
    x = torch.randn(3 * 4096 + 5, generator=g).to(DEV)
    ws = torch.empty(pkg._lib.LIMB_SCALE_WORKSPACE_BYTES, dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        out = torch.full((2,), SENTINEL, device=DEV)
        _limb_scale(pkg, x, out, ws)
        outs.append(out.cpu().view(torch.int32))
    assert torch.equal(outs[0], outs[1])
