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
