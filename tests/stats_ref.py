"""Reference and probe construction for the calibration statistics (spq_minmax_stats, spq_dynamic_limb_scale).  CPU only.

The statistics kernels reduce with min / max, so a kernel that skips part of its input still returns the right answer on random
data unless the extremum happens to lie in the skipped part.  The probes here PLANT the extrema: a background whose magnitudes lie
strictly inside the band (2^-3, 1), and per channel one value above the band and one below it, at a position the planner chooses.
All planted values are powers of two, so their log2 is an integer and the log-domain comparison is bit-exact like the linear one.

  expected()        the statistics of one batch (and the running update), straight from torch CPU amin / amax
  expected_sweep()  the same for P planted variants of one background, without P full passes (test_stats_ref_cpu proves it equal)
  *_probes()        planners: which positions get the planted values in which call, and what that covers
  check_probes()    counts that every planted extremum is the only extremum of its channel

The planners may aim at the host's slab and chunk borders (host_flat_plan, host_cols_plan).  Those two mirrors are for AIMING
ONLY: no expected value depends on them, so if the host plan changes the tests stay correct and only lose sharpness.
"""
import math
from typing import NamedTuple

import numpy as np
import torch

EPS_LOG = 2.0 ** -17            # the eps of every log-domain call: a power of two, so the clamp value and its log2 are exact
BAND_LO, BAND_HI = 2.0 ** -3, 1.0
K_MOD = 11                      # planted exponents k in 0..10: 2^(1+k) <= 2^11, 2^-(5+k) >= 2^-15 > EPS_LOG


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def background(shape, log, seed):
    """fp32 values with magnitudes strictly inside (BAND_LO, BAND_HI) and a random sign.  `log` only selects another random
    stream, so the two domains do not share data."""
    g = torch.Generator().manual_seed(2 * int(seed) + (1 if log else 0))
    n = int(math.prod(shape)) if len(shape) else 1
    mag = BAND_LO + (BAND_HI - BAND_LO) * torch.rand(n, generator=g, dtype=torch.float64)
    lo = float(np.nextafter(np.float32(BAND_LO), np.float32(1)))
    hi = float(np.nextafter(np.float32(BAND_HI), np.float32(0)))
    mag = mag.float().clamp_(lo, hi)
    sign = torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    return (mag * sign).reshape(shape)


def below_eps_background(shape, eps, seed):
    """fp32 values with |x| <= eps: magnitudes eps * [2^-3, 1], every fifth exactly eps, every seventh zero."""
    x = background(shape, True, seed).reshape(-1) * eps             # exact scaling by a power of two
    sign = torch.sign(x)
    x[::5] = sign[::5] * eps
    x[::7] = 0.0
    assert float(x.abs().max()) <= eps
    return x.reshape(shape)


def plant_values(k, log):
    """(value for the `min` position, value for the `max` position) for planted exponents k (any integer tensor).
    linear: -2^(1+k) and +2^(1+k).  log: magnitudes 2^-(5+k) and 2^(1+k), with opposite signs that alternate with k."""
    k = torch.as_tensor(k, dtype=torch.int64)
    kf = k.double()
    big = torch.pow(2.0, 1 + kf)
    if not log:
        return (-big).float(), big.float()
    s = (1 - 2 * (k % 2)).double()
    return (-s * torch.pow(2.0, -(5 + kf))).float(), (s * big).float()


# ---------------------------------------------------------------------------------------------------------------------------
# reference
# ---------------------------------------------------------------------------------------------------------------------------
def log_eps_fill(eps):
    """fp32 log2(fp32 eps): what a first log-domain batch without any |x| > eps fills both statistics with."""
    return float(torch.log2(torch.tensor(eps, dtype=torch.float32).double()).float())


def _to_log(t, eps):
    """log2(clamp(t, eps)) for t = |x| already: float64 log2 rounded to fp32.  clamp and log2 keep NaN."""
    return torch.log2(torch.clamp(t, min=eps).double()).float()


def expected(x, outer, chan, inner, per_channel, log, eps, prev=None):
    """(min, max) of one batch x viewed as [outer, chan, inner], `chan` values each (one if not per_channel), fp32.

    log: the statistics of log2(clamp(|x|, eps)); when no element has |x| > eps a first batch fills both with log2(eps) and a
    later batch leaves `prev` as it is (include/spq.h).  prev=None is a first batch (assign); otherwise prev = (min, max) of
    the batches so far and the result is torch.minimum / torch.maximum with it.  NaN propagates as in torch."""
    v = x.detach().to(torch.float32).reshape(outer, chan, inner)
    n_out = chan if per_channel else 1
    if log:
        v = v.abs()
        if not bool((v > eps).any()):
            if prev is None:
                fill = torch.full((n_out,), log_eps_fill(eps), dtype=torch.float32)
                return fill, fill.clone()
            return prev[0].clone(), prev[1].clone()
        v = _to_log(v, eps)
    if per_channel:
        lo, hi = v.amin(dim=(0, 2)), v.amax(dim=(0, 2))
    else:
        lo, hi = v.amin().reshape(1), v.amax().reshape(1)
    if prev is not None:
        lo, hi = torch.minimum(prev[0], lo), torch.maximum(prev[1], hi)
    return lo, hi


def expected_sweep(bg, outer, chan, inner, per_channel, log, eps, idx, vals):
    """expected() of a first batch for each of P variants of `bg`: variant p is bg with vals[p, :] written at the flat
    positions idx[p, :].  Returns (min [P, C], max [P, C]).

    It uses two facts instead of P full passes.  min / max over a set is the min / max of the planted values and of the
    untouched background, and the untouched background's extremum is the whole background's unless a planted position
    overwrote the element that attains it (those variants are recomputed from scratch).  fp32(log2(clamp(.))) is monotone, so
    it commutes with min / max.  No NaN may be planted here; use expected() for that."""
    assert not bool(torch.isnan(vals).any()) and not bool(torch.isnan(bg).any())
    flat = bg.reshape(-1)
    P, K = idx.shape
    C = chan if per_channel else 1
    v = flat.abs() if log else flat
    pv = vals.abs() if log else vals
    pc = (idx // inner) % chan if per_channel else torch.zeros_like(idx)
    t = v.reshape(outer, chan, inner)
    if per_channel:
        base_lo, base_hi = t.amin(dim=(0, 2)), t.amax(dim=(0, 2))
    else:
        base_lo, base_hi = t.amin().reshape(1), t.amax().reshape(1)
    lo = base_lo.expand(P, C).clone()
    hi = base_hi.expand(P, C).clone()
    lo.scatter_reduce_(1, pc, pv, "amin", include_self=True)
    hi.scatter_reduce_(1, pc, pv, "amax", include_self=True)
    over = v[idx]
    hit = ((over == base_lo[pc]) | (over == base_hi[pc])).any(dim=1)
    for p in torch.nonzero(hit).flatten().tolist():
        y = v.clone()
        y[idx[p]] = pv[p]
        y = y.reshape(outer, chan, inner)
        if per_channel:
            lo[p], hi[p] = y.amin(dim=(0, 2)), y.amax(dim=(0, 2))
        else:
            lo[p], hi[p] = y.amin().reshape(1), y.amax().reshape(1)
    if log:
        none_above = ~(hi > eps).any(dim=1)
        lo, hi = _to_log(lo, eps), _to_log(hi, eps)
        lo[none_above] = log_eps_fill(eps)
        hi[none_above] = log_eps_fill(eps)
    return lo, hi


def limb_scale_expected(max_abs):
    """{2^G, 2^-G} of include/spq.h for a tensor whose largest magnitude is max_abs: with m' = fp32(fp32(m) * fp32(1 + 2^-10))
    = f * 2^e, f in [0.5, 1), G = clamp(14 - e, -100, 100).  {1, 1} for m = 0 and for Inf."""
    m = np.float32(max_abs)
    if not (m > 0 and np.isfinite(m)):
        return np.float32(1.0), np.float32(1.0)
    guarded = np.float32(m * np.float32(1.0 + 2.0 ** -10))
    _, e = math.frexp(float(guarded))
    G = max(-100, min(100, 14 - e))
    return np.float32(2.0 ** G), np.float32(2.0 ** -G)


# ---------------------------------------------------------------------------------------------------------------------------
# host-plan mirrors -- AIMING ONLY (see the module docstring)
# ---------------------------------------------------------------------------------------------------------------------------
def _ceil_div(a, b):
    return (a + b - 1) // b


def host_flat_plan(total, cap=256):
    """AIMING ONLY: (slabs, chunk) of the per-tensor scan (cap 256) and of the limb-scale scan (cap 2048)."""
    slabs = min(cap, max(1, total // 4096))
    chunk = _ceil_div(_ceil_div(total, slabs), 4) * 4
    return _ceil_div(total, chunk), chunk


def host_cols_plan(rows):
    """AIMING ONLY: (slabs, rows_per_slab) of the column scan."""
    slabs = min(128, max(1, rows // 16))
    rps = _ceil_div(_ceil_div(rows, slabs), 4) * 4
    return _ceil_div(rows, rps), rps


def border_positions(total, chunk, chunks, radius=5):
    """Positions within `radius` of the start of each listed chunk and of its end, clipped to [0, total)."""
    out = set()
    for b in chunks:
        for edge in (b * chunk, (b + 1) * chunk):
            out.update(p for p in range(edge - radius, edge + radius + 1) if 0 <= p < total)
    return sorted(out)


def random_positions(total, n, seed):
    g = torch.Generator().manual_seed(seed)
    return sorted(set(torch.randint(0, total, (n,), generator=g).tolist()))


# ---------------------------------------------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------------------------------------------
class Probes(NamedTuple):
    """P variants of one background: variant p has vals[p, :] at flat positions idx[p, :] of x viewed as [outer, chan, inner]."""
    outer: int
    chan: int
    inner: int
    per_channel: bool
    log: bool
    bg: torch.Tensor        # flat fp32
    idx: torch.Tensor       # [P, K] int64
    vals: torch.Tensor      # [P, K] fp32
    two_sided: bool         # every channel gets a planted min AND a planted max in every variant (else only a max)
    covers: str

    def expected(self, eps=EPS_LOG):
        return expected_sweep(self.bg, self.outer, self.chan, self.inner, self.per_channel, self.log, eps, self.idx, self.vals)

    def variant(self, p):
        x = self.bg.clone()
        x[self.idx[p]] = self.vals[p]
        return x


def flat_probes(total, positions, log, seed):
    """Per-tensor statistics of `total` elements.  Variant p (p in `positions`): the min at p, the max at (p + total//2) % total,
    planted exponent k = p % 11.  total == 1 has room for one value only: the max.
    Covers: each listed position holds the tensor's sole min once and, for the positions half a tensor further, its sole max."""
    pos = torch.as_tensor(list(positions), dtype=torch.int64)
    vmin, vmax = plant_values(pos % K_MOD, log)
    if total == 1:
        idx, vals = pos.reshape(-1, 1), vmax.reshape(-1, 1)
    else:
        idx = torch.stack([pos, (pos + total // 2) % total], dim=1)
        vals = torch.stack([vmin, vmax], dim=1)
    return Probes(1, 1, total, False, log, background((total,), log, seed), idx, vals, total > 1,
                  "every listed position p holds the sole min; (p + total//2) % total holds the sole max")


def cols_probes(rows, cols, log, seed):
    """[rows, cols], one channel per column (inner == 1).  Call j: column c has its min in row (c + j*cols) % rows and its max
    rows//2 rows further (mod rows), exponent k = (c + j) % 11; ceil(rows / cols) calls.  rows == 1: only the max.
    Covers: every row holds some column's sole min and some column's sole max in at least one call; every column is planted
    in every call."""
    J = _ceil_div(rows, cols)
    j = torch.arange(J).reshape(-1, 1)
    c = torch.arange(cols).reshape(1, -1)
    min_row = (c + j * cols) % rows
    max_row = (min_row + rows // 2) % rows
    vmin, vmax = plant_values((c + j) % K_MOD, log)
    if rows == 1:
        idx, vals = max_row * cols + c, vmax
    else:
        idx = torch.cat([min_row * cols + c, max_row * cols + c], dim=1)
        vals = torch.cat([vmin, vmax], dim=1)
    return Probes(rows, cols, 1, True, log, background((rows * cols,), log, seed), idx, vals, rows > 1,
                  "every row holds a sole column min and a sole column max in some call; every column planted in every call")


def rows_probes(chan, inner, log, seed, positions=None):
    """[chan, inner], one channel per row (outer == 1).  With L = the listed positions (default: all of 0..inner-1), call j puts
    row c's min at L[(j + c) % len(L)] and its max inner//2 further (mod inner), exponent k = (c + j) % 11; len(L) calls.
    Covers: for every row, every listed position holds the row's sole min once, and the position inner//2 further its sole max."""
    L = torch.as_tensor(list(range(inner)) if positions is None else list(positions), dtype=torch.int64)
    J = len(L)
    j = torch.arange(J).reshape(-1, 1)
    c = torch.arange(chan).reshape(1, -1)
    min_pos = L[(j + c) % J]
    max_pos = (min_pos + inner // 2) % inner
    vmin, vmax = plant_values((c + j) % K_MOD, log)
    idx = torch.cat([c * inner + min_pos, c * inner + max_pos], dim=1)
    vals = torch.cat([vmin, vmax], dim=1)
    return Probes(1, chan, inner, True, log, background((chan * inner,), log, seed), idx, vals, True,
                  "for every row, every listed position holds its sole min once and the one inner//2 further its sole max")


def two_stage_probes(outer, chan, inner, log, seed):
    """[outer, chan, inner] with outer > 1 and inner > 1.  Call j: channel c has its min at (o, i) = ((c + j*chan) % outer,
    (j + c) % inner) and its max at ((o + outer//2) % outer, (i + inner//2) % inner); max(ceil(outer/chan), inner) calls.
    Covers: every outer index holds some channel's sole min and some channel's sole max in at least one call, and so does
    every inner index for every channel."""
    J = max(_ceil_div(outer, chan), inner)
    j = torch.arange(J).reshape(-1, 1)
    c = torch.arange(chan).reshape(1, -1)
    o_min = (c + j * chan) % outer
    o_max = (o_min + outer // 2) % outer
    i_min = (j + c) % inner
    i_max = (i_min + inner // 2) % inner
    vmin, vmax = plant_values((c + j) % K_MOD, log)
    idx = torch.cat([(o_min * chan + c) * inner + i_min, (o_max * chan + c) * inner + i_max], dim=1)
    vals = torch.cat([vmin, vmax], dim=1)
    return Probes(outer, chan, inner, True, log, background((outer * chan * inner,), log, seed), idx, vals, True,
                  "every outer index holds a sole channel min and max in some call; every inner index for every channel")


def any_flag_targets(rows, cols):
    """Entries of the [slabs, cols] partial-maximum array at which the lone element above eps should land: first, last, one
    below / at / above each multiple of 1024 up to 4096, and four in the tail behind the last whole 4096 (AIMING ONLY)."""
    slabs, _ = host_cols_plan(rows)
    n = slabs * cols
    t = {0, n - 1}
    for m in (1024, 2048, 3072, 4096):
        t.update((m - 1, m, m + 1))
    tail = (n // 4096) * 4096
    t.update((tail, tail + 1024, (tail + n) // 2, n - 2))
    return sorted(x for x in t if 0 <= x < n)


def any_flag_probes(rows, cols, seed):
    """[rows, cols] per column, log domain, everything at or below eps except ONE element per variant, placed (AIMING ONLY,
    through host_cols_plan) so that its slab's partial maximum is entry t of the partial array, t in any_flag_targets().
    Covers: one variant per target entry; the element is the only one above eps in the tensor."""
    _, rps = host_cols_plan(rows)
    targets = any_flag_targets(rows, cols)
    idx, ks = [], []
    for n, t in enumerate(targets):
        slab, col = divmod(t, cols)
        row = min(rows - 1, slab * rps + (7 * n) % rps)
        idx.append([row * cols + col])
        ks.append(n % K_MOD)
    _, vmax = plant_values(torch.tensor(ks), True)
    return Probes(rows, cols, 1, True, True, below_eps_background((rows * cols,), EPS_LOG, seed).reshape(-1),
                  torch.tensor(idx, dtype=torch.int64), vmax.reshape(-1, 1), False,
                  "one variant per targeted partial entry; the planted element is the only one above eps")


# magnitudes for the limb scale, all above the background band: powers of two, their fp32 neighbours, the 2^-10 guard band
# (m < 2^k <= m * (1 + 2^-10)) from inside and from just outside, and ordinary values
LIMB_MAGNITUDES = [2.0, 3.0, 32.0, float(np.nextafter(np.float32(32), np.float32(0))), float(np.nextafter(np.float32(32), np.float32(64))),
                   32.0 * (1 - 2.0 ** -12), 32.0 * (1 - 2.0 ** -9), 1.5 * 2.0 ** 20, 2.0 ** 13, 2.0 ** 14, 12345.678, 2.0 ** 90]


def limb_probes(n, positions, seed):
    """|x| maximum for spq_dynamic_limb_scale: variant p has +-LIMB_MAGNITUDES[p % len] (sign alternates every other variant)
    at the p-th listed position.  Covers: every listed position holds the sole largest magnitude once."""
    pos = torch.as_tensor(list(positions), dtype=torch.int64)
    q = torch.arange(len(pos))
    mags = torch.tensor(LIMB_MAGNITUDES, dtype=torch.float32)[q % len(LIMB_MAGNITUDES)]
    sign = (1 - 2 * ((q // 2) % 2)).float()
    return Probes(1, 1, n, False, True, background((n,), True, seed), pos.reshape(-1, 1), (mags * sign).reshape(-1, 1), False,
                  "every listed position holds the sole largest magnitude once")


def check_probes(pr, literal=48):
    """Count that the probes are what they claim.  For every variant: its positions are distinct, the background lies strictly
    inside the band (or at / below eps for the any-flag background) and, per channel, exactly one planted value lies above the
    band and (two_sided) exactly one below it -- so each planted extremum is the only extremum of its channel.  For up to
    `literal` evenly spaced variants the same is counted on the constructed tensor itself.  Returns the number of variants."""
    P, K = pr.idx.shape
    total = pr.outer * pr.chan * pr.inner
    C = pr.chan if pr.per_channel else 1
    assert pr.bg.shape == (total,) and int(pr.idx.min()) >= 0 and int(pr.idx.max()) < total
    srt = pr.idx.sort(dim=1).values
    assert K == 1 or bool((srt[:, 1:] != srt[:, :-1]).all()), "a variant plants two values at one position"
    mag = pr.bg.abs()
    top = float(mag.max())
    assert top < BAND_HI
    low_band = float(mag.min()) > BAND_LO
    assert low_band or top <= EPS_LOG
    pc = (pr.idx // pr.inner) % pr.chan if pr.per_channel else torch.zeros_like(pr.idx)
    dom = pr.vals.abs() if pr.log else pr.vals
    above = torch.zeros(P, C, dtype=torch.int64).scatter_add_(1, pc, (dom > (BAND_HI if low_band else EPS_LOG)).long())
    below = torch.zeros(P, C, dtype=torch.int64).scatter_add_(1, pc, (dom < (BAND_LO if pr.log else -BAND_HI)).long())
    planted = torch.zeros(P, C, dtype=torch.int64).scatter_add_(1, pc, torch.ones_like(pc))
    if pr.two_sided:
        assert low_band and bool((above == 1).all()) and bool((below == 1).all()) and bool((planted == 2).all())
        assert not pr.log or bool((dom > EPS_LOG).all()), "a planted small magnitude would vanish in the clamp"
    else:
        assert int(above.sum()) == P * K and bool((above <= 1).all()) and int(below.sum()) == 0
    literal = min(literal, max(2, 20_000_000 // total))
    for p in sorted(set(np.linspace(0, P - 1, min(P, literal)).astype(int).tolist())):
        x = pr.variant(p)
        v = (x.abs() if pr.log else x).reshape(pr.outer, pr.chan, pr.inner)
        if not pr.per_channel:
            v = v.reshape(1, 1, -1)
        hi, lo = v.amax(dim=(0, 2), keepdim=True), v.amin(dim=(0, 2), keepdim=True)
        n_hi, n_lo = (v == hi).sum(dim=(0, 2)), (v == lo).sum(dim=(0, 2))
        touched = planted[p] > 0
        assert bool((n_hi[touched] == 1).all()), "a planted maximum is not the only maximum of its channel"
        if pr.two_sided:
            assert bool((n_lo == 1).all()), "a planted minimum is not the only minimum of its channel"
        at = (x.abs() if pr.log else x)[pr.idx[p]]
        is_ext = (at == hi.reshape(-1)[pc[p]]) | (at == lo.reshape(-1)[pc[p]])
        assert bool(is_ext.all()), "a planted value is not an extremum of its channel"
    return P


# ---------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_calibration_stats.py (test_stats_ref_cpu.py checks the very same objects)
# ---------------------------------------------------------------------------------------------------------------------------
FLAT_TOTAL = 3 * 4096 + 5                                   # three slabs, a ragged last chunk with a scalar tail
FLAT_SMALL_TOTALS = (1, 3, 4, 5, 4095, 4097)
FLAT_CAPPED_TOTALS = (256 * 4096, 256 * 4096 + 5)
COLS_COLS = (260, 257, 64, 5)                               # VEC4 with two column blocks, scalar, one block, tiny
COLS_ROWS = (1, 3, 4, 5, 15, 16, 17, 31, 33, 321, 2048, 2100)   # 321 = 64*5 + 1: the last slab holds one row
COLS_SLAB_SWEEP = tuple(16 * s for s in list(range(1, 14)) + [127, 128, 129])
ROWS_CHAN = (1, 3, 4, 5, 260)
ROWS_INNER = (4, 7, 64, 255, 256, 257, 3072)
TWO_STAGE_SHAPES = ((6, 10, 12), (3, 5, 7), (33, 260, 4), (2049, 8, 5))
ANY_SHAPE = (2100, 260)
LIMB_N = (1, 5, 4096, 3 * 4096 + 5, 2048 * 4096 + 3)


def thinned(total, step, edge=8):
    """Every step-th position plus the first and last `edge`."""
    return sorted(set(range(0, total, step)) | set(range(min(edge, total))) | set(range(max(0, total - edge), total)))


def flat_capped_positions(total, seed):
    """+-5 around every chunk border of the first three, the middle two and the last three chunks (AIMING ONLY), the first
    and the last 600 positions, 512 seeded random ones."""
    slabs, chunk = host_flat_plan(total)
    chunks = [0, 1, 2, slabs // 2 - 1, slabs // 2, slabs - 3, slabs - 2, slabs - 1]
    pos = set(border_positions(total, chunk, chunks)) | set(range(600)) | set(range(total - 600, total))
    return sorted(pos | set(random_positions(total, 512, seed)))


def rows_long_positions(inner, seed):
    """inner = 3072: the ends, +-2 around every multiple of 256 (one wave's float4 stride), 48 seeded random positions."""
    pos = set(range(8)) | set(range(inner - 8, inner))
    for m in range(256, inner, 256):
        pos.update(range(m - 2, m + 3))
    return sorted(pos | set(random_positions(inner, 48, seed)))


def limb_positions(n, seed):
    """The ends, +-5 around the chunk borders of the first two, the middle and the last two chunks (AIMING ONLY), 64 random."""
    slabs, chunk = host_flat_plan(n, cap=2048)
    pos = set(range(min(n, 8))) | set(range(max(0, n - 8), n))
    pos |= set(border_positions(n, chunk, [0, 1, slabs // 2, slabs - 2, slabs - 1]))
    if n > 16:
        pos |= set(random_positions(n, 64, seed))
    return sorted(p for p in pos if 0 <= p < n)
