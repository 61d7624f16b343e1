"""Host reference of the log quantizer's level chain, correctly rounded, and a generator of inputs at its rounding ties.

DESIGN.md ("Log path") declares that the device decides every log level with the correctly rounded log2:

    mag = max(|x|, 1e-5f);  lg = float32(log2(float64(mag)))
    ln  = clamp(f32(lg - min) / max(range, 1e-5f), 0, 1)
    pre = ((ln - 0.5) * 2) * n   (symmetric)   |   ln * n   (asymmetric)
    q   = clamp(rint(pre), qlo, qhi)             (ties to even; NaN stays NaN)

`levels` evaluates that chain op for op in np.float32 arithmetic (numpy rounds every float32 operation once, like the
kernels' -ffp-contract=off code); only the log2 is taken in float64.  The oracle (oracle/ref_cpu.py) uses ATen's <= 1-ulp
log2 instead and so needs an allowance next to a tie; this module needs none, which is what makes it a test of the device's
fast path (v_log_f32 + v_rcp_f32 + an error bound) at the ties.

Neither numpy's float64 log2 nor the device's is correctly rounded, only faithfully: `ambiguous` marks the elements where a
2-double-ulp difference in the float64 log2 could change the float32 lg (a double rounding), and the tests leave those out and
report their count.

Pure numpy, no torch, no GPU.
"""
import numpy as np

F32 = np.float32
EPS = F32(1e-5)                     # quantization_methods.py:35, hard-coded
ZERO_MASK = F32(1e-5)               # :41

REGIONS = ("R1", "R2", "R3", "R4", "R5")


# ---------------------------------------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------------------------------------
def level_range(bits, sym):
    """(n, qlo, qhi) as the kernels' make_log_params: the multiplier before rounding and the clamp."""
    if sym:
        n = (1 << (bits - 1)) - 1
        return F32(n), F32(-n), F32(n)
    n = (1 << bits) - 1
    return F32(n), F32(0), F32(n)


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def log2_f32(mag):
    """float32(log2(float64(mag))): the correctly rounded log2 wherever `ambiguous` is false."""
    with np.errstate(divide="ignore"):
        return np.log2(_f32(mag).astype(np.float64)).astype(np.float32)


def pre_round_from_lg(lg, log_min, log_range, bits, sym):
    """log_pre_round<SYM> (spq_common.h) in float32."""
    n, _, _ = level_range(bits, sym)
    lg, log_min, log_range = _f32(lg), _f32(log_min), _f32(log_range)
    with np.errstate(invalid="ignore", over="ignore"):
        ln = (lg - log_min) / np.maximum(log_range, EPS)
        ln = np.where(np.isnan(ln), ln, np.minimum(np.maximum(ln, F32(0)), F32(1))).astype(np.float32)
        if sym:
            return (((ln - F32(0.5)) * F32(2.0)) * n).astype(np.float32)
        return (ln * n).astype(np.float32)


def pre_round(x, log_min, log_range, bits, sym):
    """The value the level is rounded from, with the correctly rounded log2."""
    x = _f32(x)
    with np.errstate(invalid="ignore"):
        mag = np.maximum(np.abs(x), EPS)                 # NaN stays NaN
    return pre_round_from_lg(log2_f32(mag), log_min, log_range, bits, sym)


def levels(x, log_min, log_range, bits, sym):
    """Integer levels (float32, NaN for a NaN input) of `x` for the given (broadcastable) log_min / log_range."""
    _, qlo, qhi = level_range(bits, sym)
    pre = pre_round(x, log_min, log_range, bits, sym)
    q = np.rint(pre)
    with np.errstate(invalid="ignore"):
        q = np.where(np.isnan(q), q, np.minimum(np.maximum(q, qlo), qhi))
    return q.astype(np.float32)


def ambiguous(x, log_min, log_range, bits, sym, ulps=2):
    """Elements whose float64 log2, moved by +-`ulps` double ulps, rounds to another float32 lg or gives another level."""
    x = _f32(x)
    with np.errstate(invalid="ignore"):
        mag = np.maximum(np.abs(x), EPS)
    return ambiguous_lg(np.log2(mag.astype(np.float64)), log_min, log_range, bits, sym, ulps)


def ambiguous_lg(lg64, log_min, log_range, bits, sym, ulps=2):
    """`ambiguous` given the float64 log2 itself (so that a double-rounding case can be constructed directly)."""
    lg64 = np.asarray(lg64, dtype=np.float64)
    lo, hi = lg64.copy(), lg64.copy()
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
    lg = lg64.astype(np.float32)
    flo, fhi = lo.astype(np.float32), hi.astype(np.float32)
    amb = (flo != lg) | (fhi != lg)                      # rounding is monotone: the two ends decide it
    plo = np.rint(pre_round_from_lg(flo, log_min, log_range, bits, sym))
    phi = np.rint(pre_round_from_lg(fhi, log_min, log_range, bits, sym))
    p = np.rint(pre_round_from_lg(lg, log_min, log_range, bits, sym))
    with np.errstate(invalid="ignore"):
        amb |= (plo != p) | (phi != p)
    return amb & ~np.isnan(lg64)


def device_err(x, log_min, log_range, bits, sym):
    """log_level's error bound (spq_common.h), evaluated in float64 from the exact lg and the exact pre-round value."""
    n, _, _ = level_range(bits, sym)
    k2 = (2.0 if sym else 1.0) * float(n)
    x = _f32(x)
    with np.errstate(invalid="ignore"):
        lg = np.log2(np.maximum(np.abs(x), EPS).astype(np.float64))
    rng = np.maximum(np.asarray(log_range, dtype=np.float64), float(EPS))
    slope = k2 / rng
    pre = pre_round(x, log_min, log_range, bits, sym).astype(np.float64)
    return 2.4e-7 * np.maximum(np.abs(lg), 1.0) * slope + 3.0e-7 * k2 + 1e-6 * np.maximum(np.abs(pre), 1.0)


def tie_distance(x, log_min, log_range, bits, sym):
    """0.5 - |pre - rint(pre)| of the correctly rounded pre-round value (0 on an exact tie)."""
    pre = pre_round(x, log_min, log_range, bits, sym).astype(np.float64)
    return 0.5 - np.abs(pre - np.rint(pre))


def coverage(x, log_min, log_range, bits, sym):
    """(elements exactly on k + 1/2, elements whose tie distance is below the device's bound) -- NaN excluded."""
    x = _f32(x)
    pre = pre_round(x, log_min, log_range, bits, sym)
    with np.errstate(invalid="ignore"):
        exact = int(np.count_nonzero(np.abs(pre - np.rint(pre)) == F32(0.5)))
        near = int(np.count_nonzero(tie_distance(x, log_min, log_range, bits, sym)
                                    < device_err(x, log_min, log_range, bits, sym)))
    return exact, near


# ---------------------------------------------------------------------------------------------------------------------------
# dequantisation: log_qn -> x_hat -> 2^x_hat * sign
# ---------------------------------------------------------------------------------------------------------------------------
def dequant(x, q, log_min, log_range, bits, sym, direct=False):
    """log_dequant<SYM> (spq_common.h) with a correctly rounded exp2: part1 (direct=False) sends the symmetric normalised level
    through * (2^b - 1) / (2^b - 1); part2's quantizer (make_log_params(direct=true)) does not."""
    n, _, _ = level_range(bits, sym)
    full = F32((1 << bits) - 1)
    x, q = _f32(x), _f32(q)
    log_min, log_range = _f32(log_min), _f32(log_range)
    with np.errstate(invalid="ignore", over="ignore"):
        if sym:
            qn = q / (F32(2.0) * n) + F32(0.5)
            if not direct:
                qn = (qn * full) / full
        else:
            qn = q / n
        x_hat = (_f32(qn) * log_range + log_min).astype(np.float32)
        mag = np.exp2(x_hat.astype(np.float64)).astype(np.float32)
        out = (mag * np.sign(x)).astype(np.float32)
    return np.where(np.abs(x) < ZERO_MASK, F32(0), out).astype(np.float32)


def ulp_distance(a, b):
    """|a - b| in float32 ulps (ordered integer view; equal NaNs 0; a NaN against a number: huge)."""
    a, b = _f32(a), _f32(b)

    def key(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a) - key(b))
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    return np.where(both_nan, 0, np.where(one_nan, 1 << 40, d))


# ---------------------------------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------------------------------
def _tie_lg(t, log_min, log_range, bits, sym):
    """float64 lg at which the exact chain's pre-round value is t."""
    n, _, _ = level_range(bits, sym)
    rng = max(float(log_range), float(EPS))
    ln = (t / float(n)) / 2.0 + 0.5 if sym else t / float(n)
    return ln * rng + float(log_min)


def _neighbours(xstar, span):
    """float32 magnitudes around each float64 xstar: the nearest float and +-1 .. +-span ulps (positive, finite, non-zero)."""
    x0 = np.asarray(xstar, dtype=np.float64).astype(np.float32).view(np.int32).astype(np.int64)
    d = np.arange(-span, span + 1, dtype=np.int64)
    b = (x0[:, None] + d[None, :]).reshape(-1)
    b = b[(b > 0) & (b < 0x7F800000)]
    return b.astype(np.int32).view(np.float32)


def tie_inputs(log_min, log_range, bits, sym, region, span=12, keep=4.0, max_ties=24, seed=0):
    """float32 inputs on and next to the rounding ties k + 1/2 of one quantizer (log_min, log_range, bits, sym).

    For each tie (at most `max_ties` of them, spread over the levels) the magnitudes around 2^lg* -- the nearest float and
    +-1 .. +-`span` ulps -- in both signs; kept are those that land exactly on a tie in the correctly rounded chain or within
    `keep` times the device's error bound of one.  `region` adds what that region is about:
      R1  ties next to lg = 0 (|x| ~ 1), where the absolute error of v_log_f32 matters;
      R2  |x| around the 1e-5 clamp and the zero mask (1e-5 and its neighbours, both signs);
      R3  large |lg| (the caller's log_min up to ~2^120 or down to 2^-16);
      R4  lg at log_min and log_min + log_range (ln at the clamp edges 0 and 1) +-span ulps, and the outermost ties;
      R5  narrow ranges (log_range near 1e-5 or 1e-3; the caller's parameters);
    and every region -0.0, +0.0 and subnormals.
    """
    assert region in REGIONS, region
    n, qlo, qhi = level_range(bits, sym)
    nb = int(qhi - qlo)                                          # boundaries qlo + 1/2 .. qhi - 1/2
    rng_ = np.random.default_rng(seed)
    if region == "R1":                                           # the boundaries nearest lg = 0
        R = max(float(log_range), float(EPS))
        ln0 = -float(log_min) / R
        p0 = (ln0 - 0.5) * 2.0 * float(n) if sym else ln0 * float(n)
        c = int(np.clip(np.floor(p0 - float(qlo)), 0, nb - 1))
        pick = np.arange(max(0, c - max_ties // 2), min(nb, c + max_ties // 2 + 1))
    elif region == "R4":
        pick = np.unique(np.r_[np.arange(min(4, nb)), nb - 1 - np.arange(min(4, nb))])
    elif nb > max_ties:
        pick = np.unique(np.r_[0, nb - 1, rng_.integers(0, nb, max_ties - 2)])
    else:
        pick = np.arange(nb)
    ts = float(qlo) + 0.5 + pick.astype(np.float64)
    lgs = _tie_lg(ts, log_min, log_range, bits, sym)
    ok = lgs < 127.5
    mags = _neighbours(np.exp2(lgs[ok]), span)
    x = np.concatenate([mags, -mags])
    t = tie_distance(x, log_min, log_range, bits, sym)
    e = device_err(x, log_min, log_range, bits, sym)
    x = x[(t == 0) | (t <= keep * e)]
    extra = [np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38], dtype=np.float32)]
    if region == "R2":
        m = _neighbours(np.array([float(EPS)]), span)
        extra += [m, -m]
    if region == "R4":
        rng = max(float(log_range), float(EPS))
        for lg in (float(log_min), float(log_min) + rng):
            if lg < 127.5:
                m = _neighbours(np.array([2.0 ** lg]), span)
                extra += [m, -m]
    allx = np.concatenate([x] + extra).astype(np.float32)
    return np.unique(allx.view(np.int32)).view(np.float32)          # by bit pattern: -0.0 and 0.0 both stay


def _log_min_for_tie(lg, log_range, bits, sym, rng, search=256):
    """A float32 log_min for which the chain puts lg (a float32) exactly on some k + 1/2; the nearest guess if none is found.
    (With a range of ~1e-5 the slope is so steep that ties are otherwise met only by chance.)"""
    n, qlo, qhi = level_range(bits, sym)
    R = max(float(log_range), float(EPS))
    for _ in range(8):
        t = float(rng.integers(int(qlo), int(qhi))) + 0.5
        ln = (t / float(n)) / 2.0 + 0.5 if sym else t / float(n)
        m0 = np.array([lg - ln * R], dtype=np.float32).view(np.int32).astype(np.int64)
        cand = (m0 + np.arange(-search, search + 1)).astype(np.int32).view(np.float32)
        pre = pre_round_from_lg(np.full(cand.shape, lg, np.float32), cand, log_range, bits, sym)
        hit = np.nonzero(pre == F32(t))[0]
        if len(hit):
            return float(cand[hit[0]])
    return float(lg - ln * R)


def region_params(region, bits, sym, count, seed=0):
    """`count` (log_min, log_range) pairs (float32) of the kind each region is about -- for the channels of a per-channel
    tie matrix.  Ranges are a mix of powers of two (where the chain is exact and ties land on k + 1/2 often) and
    calibrated-looking values."""
    rng = np.random.default_rng(seed)
    n, _, _ = level_range(bits, sym)
    out = []
    for i in range(count):
        nice = i % 2 == 0
        if region == "R1":                                       # a tie at lg ~ 0: log_min placed so that one boundary is there
            R = float(2 ** rng.integers(1, 5)) if nice else float(rng.uniform(2.0, 20.0))
            t = float(rng.integers(-int(n), int(n))) + 0.5 if sym else float(rng.integers(0, int(n))) + 0.5
            ln = (t / float(n)) / 2.0 + 0.5 if sym else t / float(n)
            m = -ln * R + float(rng.uniform(-2e-3, 2e-3)) * (0 if nice else 1)
        elif region == "R2":                                     # range starting at (or just above / below) log2(1e-5)
            R = float(2 ** rng.integers(2, 5)) if nice else float(rng.uniform(4.0, 24.0))
            m = float(np.log2(np.float64(EPS))) + float(rng.choice([0.0, -1e-3, 1e-3, -0.5, 0.25]))
        elif region == "R3":
            big = i % 4 < 2
            R = float(2 ** rng.integers(2, 4)) if nice else float(rng.uniform(3.0, 12.0))
            m = float(rng.uniform(100.0, 120.0 - R)) if big else float(rng.uniform(-16.0, -14.0))
            if nice:
                m = float(np.round(m))
        elif region == "R4":
            R = float(2 ** rng.integers(1, 5)) if nice else float(rng.uniform(2.0, 20.0))
            m = float(rng.uniform(-10.0, 4.0))
        else:                                                    # R5
            e = float(EPS)
            R = [np.nextafter(F32(e), F32(0)), F32(e), np.nextafter(F32(e), F32(1)), F32(1e-3), F32(2 ** -10)][i % 5]
            R = float(R)
            if nice:                                             # x = 1 (lg = 0 exactly) on a tie: log_min searched for it
                m = _log_min_for_tie(0.0, F32(R), bits, sym, rng)
            else:
                m = float(rng.choice([0.0, -3.3, 7.7, float(rng.uniform(-8, 8))]))
        out.append((F32(m), F32(R)))
    return out


def tie_matrix(bits, sym, chan, regions=REGIONS, rows=None, seed=0, **kw):
    """A [rows, chan] float32 tie matrix with per-channel parameters (log_min[chan], log_range[chan]): channel c is a quantizer
    of region regions[c % len(regions)] (`region_params`) and holds `tie_inputs` of its own parameters, padded with a mid-range
    value (pre-round value an integer, far from a tie).  rows=None: the longest column.  Longer columns are subsampled.
    Returns (X, log_min, log_range, region of each channel)."""
    regions = (regions,) if isinstance(regions, str) else tuple(regions)
    per = {r: iter(region_params(r, bits, sym, -(-chan // len(regions)), seed + 7 * j)) for j, r in enumerate(regions)}
    reg = [regions[c % len(regions)] for c in range(chan)]
    params = [next(per[r]) for r in reg]
    cols = [tie_inputs(m, R, bits, sym, r, seed=seed + c, **kw) for c, ((m, R), r) in enumerate(zip(params, reg))]
    if rows is None:
        rows = max(len(c) for c in cols)
    rng = np.random.default_rng(seed)
    n, _, _ = level_range(bits, sym)
    ln_mid = 0.5 if sym else float(int(n) // 2) / float(n)        # pre-round value 0 / floor(n/2)
    X = np.empty((rows, chan), dtype=np.float32)
    for c, (col, (m, R)) in enumerate(zip(cols, params)):
        if len(col) > rows:
            col = rng.choice(col, rows, replace=False)
        X[:, c] = F32(np.exp2(np.float64(m) + ln_mid * max(float(R), float(EPS))))
        X[:len(col), c] = col
    mins = np.array([p[0] for p in params], dtype=np.float32)
    ranges = np.array([p[1] for p in params], dtype=np.float32)
    return X, mins, ranges, np.array(reg)


# ---------------------------------------------------------------------------------------------------------------------------
# two-limb fp16 operands (split2 in spq_f16x2.hip) and what can be read back through them
# ---------------------------------------------------------------------------------------------------------------------------
def split2(v):
    """split2 (spq_f16x2.hip) in numpy: hi = RN_f16(v), lo = RN_f16(v - hi), the difference taken in float32."""
    v = _f32(v)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi, lo


def limb_decode(hi, lo, descale):
    """(hi + lo) * descale in float64 (exact: the limbs and the power-of-two descale lose nothing there)."""
    return (np.asarray(hi).astype(np.float64) + np.asarray(lo).astype(np.float64)) * np.asarray(descale, dtype=np.float64)


def limb_tol(v, descale):
    """What two fp16 limbs of v / descale, decoded, may be off by: 2^-22 |v| from the two roundings, plus half an f16 subnormal
    step of lo (2^-25 before the descale), both with a 2x margin -- and room for the 1-ulp (2^-23) exp2 of the device."""
    return np.abs(np.asarray(v, np.float64)) * 2.0 ** -21 + np.asarray(descale, dtype=np.float64) * 2.0 ** -24


def separable(x, q_ref, o_ref, log_min, log_range, bits, sym, direct=False, tol=None, scale=1.0):
    """Elements whose neighbouring levels dequantise (times `scale`) more than 2 * tol away from their own value -- there a
    read-back within tol pins the level.  tol=None: 2 float32 ulps (a value read back in fp32 within 1 ulp)."""
    _, qlo, qhi = level_range(bits, sym)
    ok = np.ones(np.shape(x), bool)
    for dq in (-1, 1):
        qn = np.clip(q_ref + dq, qlo, qhi)
        o_n = (dequant(x, qn, log_min, log_range, bits, sym, direct) * _f32(scale)).astype(np.float32)
        if tol is None:
            far = ulp_distance(o_n, o_ref) > 2
        else:
            far = np.abs(o_n.astype(np.float64) - np.asarray(o_ref, np.float64)) > 2 * tol
        ok &= (qn == q_ref) | far
    return ok


def ulp_pow2(v):
    """The float32 ulp of v: a power of two (v finite, normal, non-zero)."""
    _, e = np.frexp(np.abs(_f32(v)).astype(np.float64))
    return np.ldexp(1.0, e - 24).astype(np.float32)


def bias_ties(bits, sym, chan, regions=("R1", "R4"), min_lg=None, max_lg=24.0, signed=True, seed=0):
    """Per-channel quantizers and a value on one rounding tie of each, for a store that computes y = bias + q * s with an
    integer q: returns (bias, s, log_min, log_range) with bias[c] the float nearest 2^lg* of a tie of channel c and
    s[c] = ulp(bias[c]), so that q = -Q .. Q walks bias over its +-Q float neighbours.  Ties are picked at random among those
    with min_lg <= lg* <= max_lg (R1's channels: the tie at lg = 0, i.e. |x| = 1 exactly, when that is in the window); signs
    alternate when `signed`."""
    rng = np.random.default_rng(seed)
    per = {r: iter(region_params(r, bits, sym, -(-chan // len(regions)), seed + 11 * j)) for j, r in enumerate(regions)}
    _, qlo, qhi = level_range(bits, sym)
    ts = float(qlo) + 0.5 + np.arange(int(qhi - qlo), dtype=np.float64)
    lo = -120.0 if min_lg is None else float(min_lg)
    bias, mins, ranges = np.empty(chan, np.float32), np.empty(chan, np.float32), np.empty(chan, np.float32)
    for c in range(chan):
        reg = regions[c % len(regions)]
        m, R = next(per[reg])
        lgs = _tie_lg(ts, m, R, bits, sym)
        ok = np.nonzero((lgs >= lo) & (lgs <= max_lg))[0]
        if len(ok) == 0:                                         # shift the quantizer so that its lowest tie is in the window
            m = F32(float(m) + (lo - lgs.min()) + 0.25)
            lgs = _tie_lg(ts, m, R, bits, sym)
            ok = np.nonzero((lgs >= lo) & (lgs <= max_lg))[0]
        at0 = ok[np.abs(lgs[ok]) < 1e-9]
        lg = lgs[at0[0]] if (reg == "R1" and len(at0)) else lgs[rng.choice(ok)]
        b = np.float32(np.exp2(lg))
        bias[c] = -b if (signed and c % 2) else b
        mins[c], ranges[c] = m, R
    return bias, ulp_pow2(bias), mins, ranges


def walk(bias, s, Q):
    """float32(bias + q * s) for q = -Q .. Q (rows) -- the store's y when q * s is exact."""
    q = np.arange(-Q, Q + 1, dtype=np.float32)[:, None]
    return (q * s[None, :]).astype(np.float32) + bias[None, :]


def ln_ties(bits, sym, K, M, c=4.0, seed=0, **kw):
    """A LayerNorm whose output walks rounding ties: bias[k] sits on a tie of column k's quantizer (`bias_ties`) and
    weight[k] = c * ulp(bias[k]), so weight * n + bias = bias + j ulps with j ~ round(c * n) for the normalised n of a
    standard-normal row -- on the tie for |n| < 1/(2c) and on its neighbours elsewhere.  Returns (x [M, K], weight, bias,
    log_min, log_range)."""
    bias, s, mins, ranges = bias_ties(bits, sym, K, seed=seed, **kw)
    x = np.random.default_rng(seed).standard_normal((M, K)).astype(np.float32)
    return x, (F32(c) * s).astype(np.float32), bias, mins, ranges


def layernorm(x, weight, bias, eps=1e-5):
    """weight * ((x - mean) / sqrt(var + eps)) + bias with float64 statistics and the last two operations in float32 -- the
    kernel's statistics differ in the last bits (summation order); for constructing inputs, not as a bit-exact reference."""
    x64 = np.asarray(x, np.float64)
    mean = x64.mean(axis=-1, keepdims=True)
    n = ((x64 - mean) / np.sqrt(x64.var(axis=-1, keepdims=True) + eps)).astype(np.float32)
    return ((_f32(weight) * n).astype(np.float32) + _f32(bias)).astype(np.float32)
