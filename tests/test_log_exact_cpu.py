"""tests/log_exact.py against the oracle, and its tie generator against its own claims (CPU only).

log_exact is the yardstick of tests/test_gpu_log_ties.py: these tests make sure it computes the chain the oracle computes (where the
oracle's log2 is the correctly rounded one), that its inputs really sit on the rounding ties, and that its ambiguity mask sees a
double rounding."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
import log_exact as L

WIDTHS = (3, 4, 6, 8, 9, 12, 16, 18, 24)


def _random_inputs(bits, sym, chan=48, rows=512, seed=0):
    rng = np.random.default_rng(seed)
    X, mins, ranges, _ = L.tie_matrix(bits, sym, chan, seed=seed)
    noise = (rng.standard_normal((rows, chan)) * np.exp2(rng.uniform(-18, 6, (rows, chan)))).astype(np.float32)
    return np.concatenate([X, noise]), mins, ranges


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_levels_equal_the_oracle_where_its_log2_is_correctly_rounded(bits, sym):
    x, mins, ranges = _random_inputs(bits, sym, seed=bits)
    xt, mt, rt = torch.from_numpy(x), torch.from_numpy(mins)[None], torch.from_numpy(ranges)[None]
    q_oracle, pre_oracle = O.log_levels(xt, mt, rt, bits, sym)
    mag = xt.abs().clamp(min=O.LOG_FN_EPS)
    cr = (torch.log2(mag) == torch.log2(mag.double()).float()).numpy()
    assert cr.mean() > 0.99
    q = L.levels(x, mins[None], ranges[None], bits, sym)
    np.testing.assert_array_equal(q[cr], q_oracle.numpy()[cr])
    np.testing.assert_array_equal(L.pre_round(x, mins[None], ranges[None], bits, sym)[cr], pre_oracle.numpy()[cr])
    # with the oracle's transcendentals made correctly rounded, everything agrees: levels, and the dequantised values
    with O.correctly_rounded_transcendentals():
        q_cr, _ = O.log_levels(xt, mt, rt, bits, sym)
        fq_cr = O.log_fakequant(xt, mt, rt, bits, sym).numpy()
    np.testing.assert_array_equal(q, q_cr.numpy())
    np.testing.assert_array_equal(L.dequant(x, q, mins[None], ranges[None], bits, sym), fq_cr)


def test_nan_and_signed_zero():
    x = np.array([np.nan, -0.0, 0.0, -1e-45, 1e-45], np.float32)
    q = L.levels(x, np.float32(-4.0), np.float32(8.0), 4, True)
    assert np.isnan(q[0]) and (q[1:] == -7).all()                 # |x| clamped to 1e-5, below log_min: the lowest level
    d = L.dequant(x, q, np.float32(-4.0), np.float32(8.0), 4, True)
    assert np.isnan(d[0]) and (d[1:] == 0).all() and not np.signbit(d[1:]).any()


@pytest.mark.parametrize("bits", WIDTHS)
@pytest.mark.parametrize("sym", [True, False], ids=["sym", "asym"])
def test_generator_reaches_ties_in_every_region(bits, sym):
    X, mins, ranges, reg = L.tie_matrix(bits, sym, 80, seed=bits)
    for r in L.REGIONS:
        c = reg == r
        x, m, R = X[:, c], mins[None, c], ranges[None, c]
        exact, near = L.coverage(x, m, R, bits, sym)
        # the narrow ranges of R5 meet exact ties only where log_min was constructed for one (x = 1)
        assert exact >= (8 if r == "R5" else 100), (r, exact)
        assert near >= 1000, (r, near)
        # what "exact" means: the emulated pre-round value is k + 1/2 itself
        pre = L.pre_round(x, m, R, bits, sym)
        on = np.abs(pre - np.rint(pre)) == np.float32(0.5)
        assert (L.tie_distance(x, m, R, bits, sym)[on] == 0).all()
    assert int(L.ambiguous(X, mins[None], ranges[None], bits, sym).sum()) == 0


def test_generator_regions_hit_their_targets():
    bits, sym = 8, True
    m, R = np.float32(-0.37), np.float32(6.0)
    x = L.tie_inputs(m, R, bits, sym, "R1")
    lg = np.log2(np.abs(x[np.abs(x) > 1e-30]).astype(np.float64))
    assert (np.abs(lg) < 0.2).sum() > 100                                    # |x| ~ 1
    x = L.tie_inputs(np.float32(np.log2(1e-5)), np.float32(8.0), bits, sym, "R2")
    assert ((np.abs(x) >= np.float32(1e-5)) & (np.abs(x) < 1.0001e-5)).any() and ((np.abs(x) < 1e-5) & (x != 0)).any()
    x = L.tie_inputs(np.float32(110.0), np.float32(8.0), bits, sym, "R3")
    assert np.abs(x).max() > 2.0 ** 110
    m, R = np.float32(-3.0), np.float32(5.0)
    x = L.tie_inputs(m, R, bits, sym, "R4")
    lgs = L.log2_f32(np.abs(x))
    assert (lgs == m).any() and (lgs == m + R).any()                          # ln exactly 0 and exactly 1
    assert (lgs < m).any() and (lgs > m + R).any()                            # and beyond the clamp
    assert (x == 0).any() and np.signbit(x[x == 0]).any() and ((np.abs(x) < 1.2e-38) & (x != 0)).any()


def test_ambiguity_mask_catches_a_double_rounding():
    m, R, bits, sym = np.float32(-4.0), np.float32(8.0), 8, True
    a = np.float32(1.2345678)
    b = np.nextafter(a, np.float32(2))
    mid = (np.float64(a) + np.float64(b)) / 2                                 # the float32 rounding boundary between a and b
    above = np.nextafter(mid, np.inf)                                         # rounds to b; 2 double ulps lower rounds to a
    far = mid + 1e-3 * (np.float64(b) - np.float64(a))
    lg64 = np.array([above, mid, far, np.float64(a)])
    amb = L.ambiguous_lg(lg64, m, R, bits, sym)
    assert amb.tolist() == [True, True, False, False]
    assert np.float32(above) == b and np.float32(np.nextafter(np.nextafter(above, -np.inf), -np.inf)) == a
    # and on ordinary inputs it marks (almost) nothing
    x = np.random.default_rng(0).standard_normal(100000).astype(np.float32)
    assert L.ambiguous(x, m, R, bits, sym).sum() <= 2


def test_device_bound_is_the_kernels():
    """device_err is log_level's bound: at lg = 0, 8-bit symmetric, range 8 -> 2.4e-7 * 254 / 8 + 3e-7 * 254 + 1e-6."""
    e = L.device_err(np.array([1.0], np.float32), np.float32(-4.0), np.float32(8.0), 8, True)[0]
    assert e == pytest.approx(2.4e-7 * 254 / 8 + 3.0e-7 * 254 + 1e-6 * 1.0, rel=1e-12)


def test_ulp_distance():
    a = np.array([1.0, -0.0, 1.0, np.nan], np.float32)
    b = np.array([np.nextafter(np.float32(1), np.float32(2)), 0.0, np.float32(1), np.nan], np.float32)
    assert L.ulp_distance(a, b).tolist() == [1, 0, 0, 0]


def test_split2_emulation_and_limb_decoder():
    """split2's two roundings, emulated in numpy, decode to within limb_tol -- across binades, at f16 subnormals of lo and hi,
    and at the largest value a power-of-two row scale allows (2^14)."""
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.uniform(-1, 1, 20000) * np.exp2(rng.integers(-40, 14, 20000)),
                        [0.0, -0.0, 2.0 ** -24, 2.0 ** -30, 16383.99, -8192.0, 1.0 + 2.0 ** -23]]).astype(np.float32)
    hi, lo = L.split2(v)
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    d = L.limb_decode(hi, lo, 1.0)
    assert (np.abs(d - v) <= L.limb_tol(v, 1.0)).all()
    # hi is RN_f16(v), lo takes the float32 residual: exact whenever the residual fits 11 bits
    assert (hi == v.astype(np.float16)).all()
    w = (hi.astype(np.float32) + np.float32(2.0 ** -12) * np.sign(v)).astype(np.float32)   # residual of one bit
    h2, l2 = L.split2(w)
    assert (L.limb_decode(h2, l2, 1.0) == w).all()
    # a descale multiplies out exactly; without the absolute floor the decoder's bound would fail at subnormal lo
    d2 = L.limb_decode(hi, lo, 2.0 ** -20)
    assert (np.abs(d2 - v.astype(np.float64) * 2.0 ** -20) <= L.limb_tol(v.astype(np.float64) * 2.0 ** -20, 2.0 ** -20)).all()
    assert (np.abs(d - v) > np.abs(v.astype(np.float64)) * 2.0 ** -21).any()


@pytest.mark.parametrize("bits,sym,direct", [(3, True, False), (8, True, False), (12, False, False), (18, False, True)])
def test_limb_construction_reaches_the_floors(bits, sym, direct):
    """A tie matrix per output row (the weight-preparation tests' W = tie_matrix^T) keeps >= 100 exact ties and >= 1000 within the
    device bound among the elements that two fp16 limbs under a power-of-two row scale can still tell apart."""
    X, m, R, _ = L.tie_matrix(bits, sym, 48, rows=768, seed=bits)
    W = np.ascontiguousarray(X.T)
    q = L.levels(W, m[:, None], R[:, None], bits, sym)
    o = L.dequant(W, q, m[:, None], R[:, None], bits, sym, direct)
    rmax = np.abs(o).max(axis=1)
    _, e = np.frexp(rmax)
    rs = np.where(rmax > 0, np.ldexp(1.0, -np.minimum(14 - e, 126)), 1.0)       # pow2_scale_for: row max * 2^e in [2^13, 2^14)
    hi, lo = L.split2((o / rs[:, None]).astype(np.float32))
    tol = L.limb_tol(o, rs[:, None])
    assert (np.abs(L.limb_decode(hi, lo, rs[:, None]) - o) <= tol).all()
    sep = L.separable(W, q, o, m[:, None], R[:, None], bits, sym, direct, tol=tol)
    exact, near = L.coverage(np.where(sep, W, np.float32(np.nan)), m[:, None], R[:, None], bits, sym)
    assert exact >= 100 and near >= 1000, (exact, near)


@pytest.mark.parametrize("bits,sym,min_lg", [(4, True, None), (8, False, None), (16, True, None), (8, True, 3.0), (13, False, 3.0)])
def test_bias_construction_reaches_the_floors(bits, sym, min_lg):
    """bias_ties + walk: y = bias + q ulp(bias) lands on and around a tie of every channel; with min_lg = 3 (the GELU store's
    window, where gelu is the identity in fp32) every y is above 8.  Decoded through limbs under one 2^-G, the floors hold."""
    bias, s, m, R = L.bias_ties(bits, sym, 512, min_lg=min_lg, max_lg=20.0, signed=min_lg is None, seed=bits)
    assert (s == L.ulp_pow2(bias)).all() and (np.log2(s) == np.round(np.log2(s))).all()
    y = L.walk(bias, s, 127)
    np.testing.assert_array_equal(y[127], bias)
    assert (np.unique(y.view(np.int32), axis=0).shape[0]) == 255                  # 255 distinct rows: the neighbours
    if min_lg is not None:
        assert (y > 8.0).all()
    q = L.levels(y, m[None], R[None], bits, sym)
    o = L.dequant(y, q, m[None], R[None], bits, sym)
    G = 13 - int(np.ceil(np.log2(np.abs(o).max())))
    tol = L.limb_tol(o, 2.0 ** -G)
    sep = L.separable(y, q, o, m[None], R[None], bits, sym, tol=tol)
    exact, near = L.coverage(np.where(sep, y, np.float32(np.nan)), m[None], R[None], bits, sym)
    assert exact >= 100 and near >= 1000, (exact, near)
    assert int(L.ambiguous(y, m[None], R[None], bits, sym).sum()) <= 4


@pytest.mark.parametrize("K,bits,sym", [(128, 4, True), (128, 8, False), (256, 12, True), (128, 16, False), (128, 6, True)])
def test_layernorm_construction_reaches_the_floors(K, bits, sym):
    """ln_ties: bias on a tie of each column, weight a few ulps of it -- the normalised rows land on and around the ties, and the
    floors hold among the elements the activation pass's limbs (2^-20 relative, 2^-36 of the largest value) can tell apart."""
    x, w, b, m, R = L.ln_ties(bits, sym, K, 2048, seed=K + bits, max_lg=20.0)
    y = L.layernorm(x, w, b)
    steps = np.rint((y - b[None]) / L.ulp_pow2(b)[None])
    assert np.abs(steps).max() <= 24 and (steps == 0).mean() > 0.05                # y = bias + a few ulps, often bias itself
    q = L.levels(y, m[None], R[None], bits, sym)
    o = L.dequant(y, q, m[None], R[None], bits, sym)
    tol = np.abs(o) * 2.0 ** -20 + np.exp2(np.max(m.astype(np.float64) + R)) * 2.0 ** -36
    sep = L.separable(y, q, o, m[None], R[None], bits, sym, tol=tol)
    exact, near = L.coverage(np.where(sep, y, np.float32(np.nan)), m[None], R[None], bits, sym)
    assert exact >= 100 and near >= 1000, (exact, near)
