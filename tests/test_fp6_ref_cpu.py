"""CPU: the numpy reference of the FP6 operand format (tests/fp6_ref.py) and the host-side argument checks of SPQ_PATH_FP6."""
import ctypes
import os

import numpy as np
import pytest

import fp6_ref as F6


def test_e2m3_round_trip_levels_and_digits():
    q = np.arange(-7, 8)
    assert np.array_equal(F6.e2m3_decode(F6.encode_level(q)), q.astype(np.float64))
    d = np.arange(-16, 17)
    assert np.array_equal(F6.e2m3_decode(F6.encode_digit(d)) * 8.0, d.astype(np.float64))
    # the codes the format comment states: 1.0 = 0x08, 7.0 = 0x1E, 2.0 = 0x10, 1/8 = 0x01; the sign is bit 5
    assert F6.encode_level(1) == 0x08 and F6.encode_level(7) == 0x1E and F6.encode_digit(16) == 0x10 and F6.encode_digit(1) == 0x01
    assert F6.encode_level(-3) == (0x20 | F6.encode_level(3))
    assert len(set(F6.e2m3_decode(np.arange(64)).tolist())) == 63          # +-0 coincide, every other code is a distinct number
    with pytest.raises(ValueError):
        F6.encode_level(8)


def test_digit_decomposition():
    rng = np.random.default_rng(0)
    top = (1 << 24)
    w = np.concatenate([
        rng.integers(-top, top + 1, size=200000),
        np.array([0, 1, -1, top - 1, -(top - 1), top, -top, 16, -16, 17, -17, 31, 32, 33, 496, 528]),
        # runs of digits at +-16 and the carries next to them
        np.array([sum(16 * 32 ** i for i in range(n)) for n in range(1, 5)]),
        np.array([sum(16 * 32 ** i for i in range(n)) + 1 for n in range(1, 5)]),
        -np.array([sum(16 * 32 ** i for i in range(n)) for n in range(1, 5)]),
        np.array([sum(17 * 32 ** i for i in range(n)) for n in range(1, 5)]),
        np.array([32 ** i * 16 + s for i in range(5) for s in (-1, 0, 1) if 32 ** i * 16 + s <= top]),
    ])
    d = F6.digits_of(w)
    assert d.shape == w.shape + (5,)
    assert np.array_equal(F6.from_digits(d), w)
    assert int(np.abs(d).max()) == 16
    F6.encode_digit(d)                                                        # every digit is an e2m3 number of eighths
    with pytest.raises(ValueError):
        F6.digits_of(np.array([17318417]))                                    # one past the range of five digits


def test_row_exponent_rule():
    rng = np.random.default_rng(1)
    wp = rng.standard_normal((64, 100)) * np.exp2(rng.integers(-30, 30, size=(64, 1)))
    wp[5] = 0.0
    wp[6, :] = 0.0; wp[6, 3] = 2.0 ** -7                                      # a power of two sits at the lower edge
    wp[7, 0] = np.nextafter(1.0, 0.0)
    E = F6.row_exponent(wp)
    mx = np.abs(wp).max(axis=1) * np.exp2(E.astype(np.float64))
    live = np.abs(wp).max(axis=1) > 0
    assert np.all((mx[live] >= 2.0 ** 23) & (mx[live] < 2.0 ** 24))
    assert E[5] == 0 and mx[6] == 2.0 ** 23
    w = F6.weight_integers(wp, E)
    assert int(np.abs(w).max()) <= 1 << 24
    assert np.array_equal(F6.weight_integers(np.array([[0.5, 1.5, 2.5, 8388607.0]]), np.array([0])), [[0, 2, 2, 8388607]])   # ties to even


@pytest.mark.parametrize("rows,K,row_pad", [(32, 128, 32), (70, 72, 32), (100, 72, 128), (1, 1, 32), (33, 129, 32), (257, 320, 256), (128, 3072, 128)])
def test_pack_unpack_ragged(rows, K, row_pad):
    rng = np.random.default_rng(rows * 1000 + K)
    codes = rng.integers(0, 64, size=(rows, K)).astype(np.uint8)
    buf = F6.pack(codes, row_pad)
    assert buf.size == F6.plane_bytes(rows, K, row_pad) and buf.size % F6.PAIR_BYTES == 0
    assert np.array_equal(F6.unpack(buf, rows, K, row_pad), codes)
    full = F6.unpack_full(buf, rows, K, row_pad)
    assert not full[rows:].any() and not full[:, K:].any()                    # zero padding


def test_pack_field_placement():
    """one code at (row 21, k 167): pair 0, rec 1, row-in-rec 5, k block 1, k quarter 1, position 7 -> lane 21, bit 42 of the field"""
    codes = np.zeros((32, 256), dtype=np.uint8)
    codes[21, 167] = 0x3F
    buf = F6.pack(codes).reshape(2, F6.PAIR_BYTES)
    assert not buf[0].any()
    want = np.zeros(F6.PAIR_BYTES, dtype=np.uint8)
    want[1024 + 21 * 16 + 5] = 0xFC                                           # bits 42..47 = byte 5, bits 2..7
    assert np.array_equal(buf[1], want)
    codes[:] = 0; codes[3, 31] = 0x3F                                         # the last code of a field: bits 186..191 = byte 23 -> 8-B part, byte 7
    buf = F6.pack(codes).reshape(2, F6.PAIR_BYTES)
    want[:] = 0; want[2048 + 3 * 8 + 7] = 0xFC
    assert np.array_equal(buf[0], want)


def test_weight_pack_round_trip():
    rng = np.random.default_rng(7)
    wp = rng.standard_normal((100, 72)) * 0.03
    wp[11] = 0.0
    planes, E = F6.pack_weight(wp)
    assert planes.shape == (5, F6.plane_bytes(100, 72, 128))
    assert np.array_equal(F6.unpack_weight(planes, 100, 72), F6.weight_integers(wp, E))


# ---- host-side checks of the C ABI (no HIP call is reached)
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import llm_qat_on_gpt2_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        g.build()
    return pkg._lib.load()


def test_path_constants():
    import llm_qat_on_gpt2_amd as pkg
    assert pkg._lib.PATH_FP6 == 6 and pkg._lib.PATH_NAMES[6] == "fp6"


def test_fp6_sizes_positive_and_monotone(lib):
    import llm_qat_on_gpt2_amd as pkg
    P = pkg._lib.PATH_FP6
    base = (300, 72, 100, 16)
    w0, p0 = lib.spq_fwd_workspace_bytes(*base, P), lib.spq_prep_bytes(base[2], base[1], base[3], P)
    assert w0 > 0 and p0 > 0
    assert lib.spq_fwd_workspace_bytes(0, 72, 100, 16, P) == 0 and lib.spq_prep_bytes(0, 72, 16, P) == 0
    for M in (1, 31, 32, 255, 256, 257, 8192):
        for K in (1, 64, 72, 128, 129, 768, 3072):
            ws = lib.spq_fwd_workspace_bytes(M, K, 100, 16, P)
            # the packed level plane of ceil(M/256)*256 rows at offset 0, then LoRA limbs and row scales
            assert ws >= F6.plane_bytes(M, K, 256)
            assert lib.spq_fwd_workspace_bytes(M + 256, K, 100, 16, P) > ws
            assert lib.spq_fwd_workspace_bytes(M, K + 128, 100, 16, P) > ws
            assert lib.spq_fwd_workspace_bytes(M, K, 100 + 128, 16, P) >= ws
            assert lib.spq_fwd_workspace_bytes(M, K, 100, 16 + 64, P) > ws
    for N in (1, 100, 128, 129, 3072):
        for K in (1, 72, 128, 129, 768):
            pb = lib.spq_prep_bytes(N, K, 16, P)
            assert pb >= 5 * F6.plane_bytes(N, K, 128)
            assert lib.spq_prep_bytes(N + 128, K, 16, P) > pb and lib.spq_prep_bytes(N, K + 128, 16, P) > pb
            assert lib.spq_prep_bytes(N, K, 16 + 64, P) > pb
    assert lib.spq_debug_split_k(8192, 3072, 768, 64, P) == 1


def _fwd_args(pkg, **kw):
    a = pkg._lib.FwdArgs(M=256, K=128, N=128, r=16, bits=4, qtype=0, symmetric=1, quantize_input=1, x_per_channel=1, path=pkg._lib.PATH_FP6)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,word", [
    (dict(bits=8), b"2..4 bits"),
    (dict(bits=1), b"2..4 bits"),
    (dict(qtype=1), b"symmetric minmax"),
    (dict(symmetric=0), b"symmetric minmax"),
    (dict(quantize_input=0), b"symmetric minmax"),
    (dict(lora_on_fq_input=1), b"lora_on_fq_input"),
    (dict(out_levels=0x1000, out_bits=4), b"levels-out"),
    (dict(epilogue=1, N=130), b"GELU"),
    (dict(r=129), b"rank"),
])
def test_fp6_invalid_combinations_refused(lib, kw, word):
    """refused with SPQ_ERR_UNSUPPORTED and a reason, before any pointer is looked at (all operand pointers here are null)"""
    import llm_qat_on_gpt2_amd as pkg
    rc = lib.spq_linear_lora_fwd(ctypes.byref(_fwd_args(pkg, **kw)), None)
    assert rc == -3, (rc, lib.spq_last_error())
    assert word in lib.spq_last_error(), lib.spq_last_error()


def test_fp6_valid_combination_passes_the_path_check(lib):
    """the same call with a valid combination gets past the path check and fails on its null operands instead (SPQ_ERR_INVALID)"""
    import llm_qat_on_gpt2_amd as pkg
    rc = lib.spq_linear_lora_fwd(ctypes.byref(_fwd_args(pkg)), None)
    assert rc == -1 and b"null operand" in lib.spq_last_error()
