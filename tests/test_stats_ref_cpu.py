"""tests/stats_ref.py checked on the CPU: the reference against a brute-force float64 loop, every planner's coverage claim by
counting, and that each planted extremum is the only extremum of its channel.  Without these the GPU file
(test_gpu_calibration_stats.py) would prove less than it says."""
import math

import numpy as np
import pytest
import torch

import stats_ref as R

EPS = R.EPS_LOG
NAN = float("nan")


# ---- expected() against a brute-force loop -----------------------------------------------------------------------------
def _brute(x, outer, chan, inner, per_channel, log, eps, prev=None):
    """Plain Python over float64 values; a NaN anywhere in a channel makes both of its statistics NaN (as torch does)."""
    v = [float(t) for t in x.reshape(-1).tolist()]
    groups = {}
    for n, t in enumerate(v):
        groups.setdefault((n // inner) % chan if per_channel else 0, []).append(t)
    n_out = chan if per_channel else 1
    if log and not any(abs(t) > eps for t in v):
        if prev is None:
            return [np.float32(math.log2(eps))] * n_out, [np.float32(math.log2(eps))] * n_out
        return list(prev[0]), list(prev[1])
    lo, hi = [], []
    for c in range(n_out):
        g = groups[c]
        if any(t != t for t in g):
            lo.append(np.float32(NAN)); hi.append(np.float32(NAN))
            continue
        if log:
            g = [np.float32(math.log2(max(abs(t), eps))) for t in g]
        lo.append(np.float32(min(g))); hi.append(np.float32(max(g)))
    if prev is not None:
        for c in range(n_out):
            a, b = float(prev[0][c]), float(prev[1][c])
            lo[c] = np.float32(NAN) if (a != a or lo[c] != lo[c]) else np.float32(min(a, float(lo[c])))
            hi[c] = np.float32(NAN) if (b != b or hi[c] != hi[c]) else np.float32(max(b, float(hi[c])))
    return lo, hi


def _same(t, ref):
    a, b = t.numpy().view(np.int32), np.asarray(ref, dtype=np.float32)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(t.numpy()), nan) and np.array_equal(a[~nan], b.view(np.int32)[~nan])


@pytest.mark.parametrize("shape", [(2, 3, 4), (1, 5, 3), (4, 1, 2), (3, 4, 1)])
@pytest.mark.parametrize("per_channel", [True, False])
@pytest.mark.parametrize("log", [False, True])
def test_expected_matches_brute_force(shape, per_channel, log):
    g = torch.Generator().manual_seed(sum(shape) + 2 * log)
    x = torch.randn(shape, generator=g) * 3
    x.reshape(-1)[1] = 0.0
    x.reshape(-1)[2] = EPS / 2          # clamped in the log domain
    x.reshape(-1)[3] = -EPS             # exactly eps: not "above eps", clamps to itself
    got = R.expected(x, *shape, per_channel, log, EPS)
    ref = _brute(x, *shape, per_channel, log, EPS)
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    # a second, narrower batch and a third with a NaN: merge rules
    x2 = x * 0.5
    got2 = R.expected(x2, *shape, per_channel, log, EPS, prev=got)
    ref2 = _brute(x2, *shape, per_channel, log, EPS, prev=ref)
    assert _same(got2[0], ref2[0]) and _same(got2[1], ref2[1])
    x3 = x.clone()
    x3.reshape(-1)[-1] = NAN
    got3 = R.expected(x3, *shape, per_channel, log, EPS, prev=got2)
    ref3 = _brute(x3, *shape, per_channel, log, EPS, prev=ref2)
    assert _same(got3[0], ref3[0]) and _same(got3[1], ref3[1])
    assert bool(torch.isnan(got3[0]).any()) and int(torch.isnan(got3[0]).sum()) == (1 if per_channel and shape[1] > 1 else got3[0].numel())
    # NaN is sticky
    got4 = R.expected(x2, *shape, per_channel, log, EPS, prev=got3)
    assert torch.equal(torch.isnan(got4[0]), torch.isnan(got3[0])) and torch.equal(torch.isnan(got4[1]), torch.isnan(got3[1]))


@pytest.mark.parametrize("per_channel", [True, False])
def test_expected_eps_rules(per_channel):
    shape = (3, 4, 2)
    n_out = 4 if per_channel else 1
    x = R.below_eps_background(shape, EPS, 1)
    assert float(x.abs().max()) == EPS                                  # some elements exactly at eps: still "none above"
    fill = torch.full((n_out,), -17.0)
    lo, hi = R.expected(x, *shape, per_channel, True, EPS)
    assert torch.equal(lo, fill) and torch.equal(hi, fill) and R.log_eps_fill(EPS) == -17.0
    prev = (torch.full((n_out,), -3.25), torch.full((n_out,), 7.5))
    lo, hi = R.expected(x, *shape, per_channel, True, EPS, prev=prev)
    assert torch.equal(lo, prev[0]) and torch.equal(hi, prev[1])        # a later batch: untouched
    y = x.clone()
    y[1, 2, 0] = -8.0                                                   # one element above eps: every channel is updated
    lo, hi = R.expected(y, *shape, per_channel, True, EPS)
    ref = _brute(y, *shape, per_channel, True, EPS)
    assert _same(lo, ref[0]) and _same(hi, ref[1])
    assert float(hi[2 if per_channel else 0]) == 3.0 and bool((lo == -17.0).all())
    # the linear domain has no such rule
    lo, hi = R.expected(x, *shape, per_channel, False, EPS)
    ref = _brute(x, *shape, per_channel, False, EPS)
    assert _same(lo, ref[0]) and _same(hi, ref[1])


def test_background_and_planted_values():
    for log in (False, True):
        b = R.background((5000,), log, 3)
        assert b.dtype == torch.float32 and float(b.abs().min()) > R.BAND_LO and float(b.abs().max()) < R.BAND_HI
        assert 0.4 < float((b > 0).float().mean()) < 0.6
        k = torch.arange(R.K_MOD)
        vmin, vmax = R.plant_values(k, log)
        for v in (vmin, vmax):
            m, e = np.frexp(v.abs().numpy())
            assert np.all(m == 0.5)                                     # exact powers of two
        if log:
            assert bool((vmax.abs() > R.BAND_HI).all()) and bool((vmin.abs() < R.BAND_LO).all()) and bool((vmin.abs() > EPS).all())
            assert bool((torch.sign(vmin) == -torch.sign(vmax)).all()) and len(set(torch.sign(vmax).tolist())) == 2
        else:
            assert bool((vmax > R.BAND_HI).all()) and bool((vmin < -R.BAND_HI).all())
        assert len(set(vmax.abs().tolist())) == R.K_MOD and len(set(vmin.abs().tolist())) == R.K_MOD
    assert not torch.equal(R.background((64,), False, 3), R.background((64,), True, 3))


# ---- expected_sweep() == expected() of every variant ---------------------------------------------------------------------
def _small_probe_sets():
    for log in (False, True):
        yield R.flat_probes(37, range(37), log, 1)
        yield R.flat_probes(1, range(1), log, 2)
        yield R.cols_probes(7, 5, log, 3)
        yield R.cols_probes(1, 6, log, 4)
        yield R.rows_probes(3, 7, log, 5)
        yield R.two_stage_probes(3, 5, 7, log, 6)
    yield R.any_flag_probes(40, 12, 7)
    yield R.limb_probes(5, range(5), 8)              # plants on top of the background's own extremum: the recomputed variants
    yield R.limb_probes(40, range(40), 9)


def test_expected_sweep_equals_expected_of_each_variant():
    recomputed = 0
    for pr in _small_probe_sets():
        lo, hi = pr.expected()
        over = (pr.bg.abs() if pr.log else pr.bg)[pr.idx]
        ext = pr.bg.abs() if pr.log else pr.bg
        for p in range(pr.idx.shape[0]):
            e_lo, e_hi = R.expected(pr.variant(p), pr.outer, pr.chan, pr.inner, pr.per_channel, pr.log, EPS)
            assert torch.equal(lo[p], e_lo) and torch.equal(hi[p], e_hi), (pr.covers, p)
        if not pr.per_channel:
            recomputed += int(((over == ext.max()) | (over == ext.min())).any(dim=1).sum())
    assert recomputed > 0                             # the from-scratch branch was exercised too


def test_expected_sweep_fills_when_nothing_is_above_eps():
    bg = R.below_eps_background((6, 4), EPS, 2).reshape(-1)
    idx = torch.tensor([[3], [9]])
    vals = torch.tensor([[EPS / 4], [-4.0]])
    lo, hi = R.expected_sweep(bg, 6, 4, 1, True, True, EPS, idx, vals)
    assert bool((lo[0] == -17.0).all()) and bool((hi[0] == -17.0).all())
    assert float(hi[1, 1]) == 2.0 and int((hi[1] == -17.0).sum()) == 3


# ---- the planners of the GPU file: coverage by counting, uniqueness of every planted extremum ------------------------------
def _halves(pr):
    K = pr.idx.shape[1]
    return pr.idx[:, : K // 2], pr.idx[:, K // 2:]


@pytest.mark.parametrize("log", [False, True])
def test_flat_planner_covers_every_position(log):
    T = R.FLAT_TOTAL
    pr = R.flat_probes(T, range(T), log, 11)
    assert R.check_probes(pr) == T
    assert torch.equal(pr.idx[:, 0].sort().values, torch.arange(T)) and torch.equal(pr.idx[:, 1].sort().values, torch.arange(T))
    assert len(set((pr.idx[:, 0] % R.K_MOD).tolist())) == R.K_MOD
    for total in R.FLAT_SMALL_TOTALS:
        pos = R.thinned(total, 3)
        pr = R.flat_probes(total, pos, log, 12)
        assert R.check_probes(pr) == len(pos)
        assert {0, total - 1} <= set(pos) and (total > 8 or pos == list(range(total)))
    for total in R.FLAT_CAPPED_TOTALS:
        pos = R.flat_capped_positions(total, 13)
        pr = R.flat_probes(total, pos, log, 14)
        assert R.check_probes(pr) == len(pos)
        slabs, chunk = R.host_flat_plan(total)
        assert slabs == 256 and set(range(600)) <= set(pos) and set(range(total - 600, total)) <= set(pos)
        for b in (1, 2, 3, slabs // 2, slabs - 2, slabs - 1):            # both sides of these chunk borders
            assert {b * chunk - 1, b * chunk} <= set(pos)
        assert len(pos) >= 1200 + 512


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("cols", R.COLS_COLS + (68,))
def test_cols_planner_covers_every_row_and_column(cols, log):
    for rows in sorted(set(R.COLS_ROWS + R.COLS_SLAB_SWEEP)):
        pr = R.cols_probes(rows, cols, log, 21)
        assert R.check_probes(pr, literal=4) == -(-rows // cols)
        mn, mx = _halves(pr) if rows > 1 else (pr.idx, pr.idx)
        for half in (mn, mx):
            assert torch.equal(half % cols, torch.arange(cols).expand_as(half))          # every column in every call
            seen = torch.bincount((half // cols).reshape(-1), minlength=rows)
            assert seen.numel() == rows and int(seen.min()) >= 1, (rows, cols)            # every row at least once
    slabs, rps = R.host_cols_plan(321)
    assert 321 - (slabs - 1) * rps == 1                                                   # the short last slab of the issue
    # 16 * 129 rows exceed the cap of 128 slabs: 20 rows per slab after rounding up to a multiple of 4, so 104 slabs
    assert [R.host_cols_plan(r)[0] for r in R.COLS_SLAB_SWEEP] == list(range(1, 14)) + [127, 128, 104]


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("chan", R.ROWS_CHAN)
def test_rows_planner_covers_every_position_of_every_row(chan, log):
    for inner in R.ROWS_INNER:
        L = None if inner <= 257 else R.rows_long_positions(inner, 31)
        pr = R.rows_probes(chan, inner, log, 32, L)
        listed = list(range(inner)) if L is None else L
        assert R.check_probes(pr, literal=4) == len(listed)
        mn, mx = _halves(pr)
        for c in range(chan):
            assert sorted((mn[:, c] - c * inner).tolist()) == listed                      # each listed position exactly once
            assert sorted((mx[:, c] - c * inner).tolist()) == sorted((p + inner // 2) % inner for p in listed)
        if L is not None:
            assert {0, inner - 1, 255, 256, 257, inner - 256} <= set(L)


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("shape", R.TWO_STAGE_SHAPES)
def test_two_stage_planner_covers_outer_and_inner(shape, log):
    outer, chan, inner = shape
    pr = R.two_stage_probes(outer, chan, inner, log, 41)
    R.check_probes(pr, literal=4)
    for half in _halves(pr):
        c = (half // inner) % chan
        assert torch.equal(c, torch.arange(chan).expand_as(c))
        o, i = half // (inner * chan), half % inner
        assert int(torch.bincount(o.reshape(-1), minlength=outer).min()) >= 1
        for ch in range(chan):
            assert int(torch.bincount(i[:, ch], minlength=inner).min()) >= 1


def test_any_flag_planner_hits_its_targets():
    rows, cols = R.ANY_SHAPE
    pr = R.any_flag_probes(rows, cols, 51)
    targets = R.any_flag_targets(rows, cols)
    assert R.check_probes(pr, literal=4) == len(targets)
    slabs, rps = R.host_cols_plan(rows)
    n = slabs * cols
    assert n > 4096 and {0, n - 1, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097} <= set(targets)
    assert sum(t >= (n // 4096) * 4096 for t in targets) >= 4                             # behind the last whole 4 x 1024
    rc = pr.idx.reshape(-1)
    assert ((rc // cols) // rps * cols + rc % cols).tolist() == targets                   # the aim, through the mirror
    lo, hi = pr.expected()
    assert bool((lo == -17.0).all()) and int((hi != -17.0).sum()) == len(targets)         # one channel per variant gets the planted log
    assert bool((hi[torch.arange(len(targets)), rc % cols] >= 1.0).all())


def test_limb_planner_and_positions():
    for n in R.LIMB_N:
        pos = R.limb_positions(n, 61)
        pr = R.limb_probes(n, pos, 62)
        assert R.check_probes(pr) == len(pos)
        assert pr.idx.reshape(-1).tolist() == pos and {0, n - 1} <= set(pos)
        assert n <= 16 or len(pos) >= 64
        if n > 16:
            assert len(set(pr.vals.abs().reshape(-1).tolist())) == len(R.LIMB_MAGNITUDES) and bool((pr.vals < 0).any()) and bool((pr.vals > 0).any())
    slabs, chunk = R.host_flat_plan(R.LIMB_N[-1], cap=2048)
    assert slabs > 2040                                                                   # the capped plan


# ---- limb_scale_expected ---------------------------------------------------------------------------------------------------
def test_limb_scale_expected_hand_picked():
    f32 = np.float32
    below32, above32 = np.nextafter(f32(32), f32(0)), np.nextafter(f32(32), f32(64))
    cases = [
        (1.0, 13), (1.5, 13), (2.0, 12), (3.0, 12), (32.0, 8), (above32, 8),
        (below32, 8),                       # inside the guard: 32 (1 - 2^-24) (1 + 2^-10) >= 32 -> scaled like 32
        (32.0 * (1 - 2.0 ** -12), 8),       # inside the guard
        (32.0 * (1 - 2.0 ** -9), 9),        # outside it: still the binade below
        (2.0 ** 13, 0), (2.0 ** 14, -1), (2.0 ** -20, 33),
        (2.0 ** -120, 100), (2.0 ** 120, -100),   # G clamps at +-100
    ]
    for m, G in cases:
        p, q = R.limb_scale_expected(m)
        assert (float(p), float(q)) == (2.0 ** G, 2.0 ** -G), (m, G)
        assert p.dtype == np.float32 and f32(1) / p == q
        if abs(G) < 100:
            guarded = float(f32(f32(m) * f32(1 + 2.0 ** -10))) * float(p)
            assert 2.0 ** 13 <= guarded < 2.0 ** 14 and float(f32(m)) * float(p) < 2.0 ** 14
    # the guard's edge: the largest m whose guarded product stays below 32, and its successor
    m = f32(32.0 / (1 + 2.0 ** -10))
    while f32(m * f32(1 + 2.0 ** -10)) >= 32:
        m = np.nextafter(m, f32(0))
    assert float(R.limb_scale_expected(m)[0]) == 2.0 ** 9 and float(R.limb_scale_expected(np.nextafter(m, f32(64)))[0]) == 2.0 ** 8
    for m in (0.0, -0.0, float("inf")):
        assert tuple(map(float, R.limb_scale_expected(m))) == (1.0, 1.0)
    for m in R.LIMB_MAGNITUDES:
        p, q = R.limb_scale_expected(m)
        assert float(p) * float(q) == 1.0 and float(f32(m)) * float(p) < 2.0 ** 14
