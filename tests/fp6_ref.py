"""Numpy reference of the FP6 (e2m3) operand format of SPQ_PATH_FP6 (test infrastructure; independent of the device code).

e2m3: 1 sign, 2 exponent (bias 1), 3 mantissa bits; every multiple of 1/8 up to 2.0 and every integer up to 7 is a number; no
NaN / Inf.  A packed plane holds a [rows, K] matrix of 6-bit codes in MFMA-operand-tile order: rows in pairs of 32, k in blocks
of 128 (k padded with the zero code); one (pair, k block) = 3072 B = [rec0 16-B parts 1 KB | rec1 16-B parts 1 KB | rec0 8-B
parts 512 B | rec1 8-B parts 512 B], rec = 16 rows; lane l = (row & 15) + 16 (k / 32 % 4) owns a 24-B field = its row's 32 codes
of k = 32 (l >> 4) .. + 31, 6 bits each, LSB first: bytes 0..15 in the 16-B part, bytes 16..23 in the 8-B part.
"""
import numpy as np

PAIR_BYTES = 3072
NDIGITS = 5


def e2m3_decode(code):
    """code (0..63) -> value (float64)"""
    code = np.asarray(code).astype(np.int64)
    sign = np.where(code & 0x20, -1.0, 1.0)
    e, m = (code >> 3) & 3, code & 7
    mag = np.where(e == 0, m / 8.0, (1.0 + m / 8.0) * np.exp2(e - 1.0))
    return sign * mag


_TABLE = e2m3_decode(np.arange(64))


def e2m3_encode(v):
    """exactly representable value -> code (raises if a value is no e2m3 number); -0 is not produced"""
    v = np.asarray(v, dtype=np.float64)
    code = np.full(v.shape, -1, dtype=np.int64)
    for c in range(64):
        if c == 0x20:
            continue                                         # negative zero
        code = np.where(v == _TABLE[c], c, code)
    if (code < 0).any():
        raise ValueError("value not representable in e2m3")
    return code.astype(np.uint8)


def encode_level(q):
    """integer activation level |q| <= 7"""
    return e2m3_encode(np.asarray(q, dtype=np.float64))


def encode_digit(d):
    """weight digit |d| <= 16, stored as d / 8"""
    return e2m3_encode(np.asarray(d, dtype=np.float64) / 8.0)


def plane_bytes(rows, K, row_pad=32):
    rp = -(-rows // row_pad) * row_pad
    return (rp // 32) * (-(-K // 128)) * PAIR_BYTES


def pack(codes, row_pad=32):
    """codes uint8 [rows, K] -> packed plane (uint8, 1-D); rows padded to row_pad, K to 128, with the zero code"""
    codes = np.asarray(codes, dtype=np.uint8)
    rows, K = codes.shape
    rp, kp = -(-rows // row_pad) * row_pad, -(-K // 128) * 128
    full = np.zeros((rp, kp), dtype=np.uint8)
    full[:rows, :K] = codes
    KB = kp // 128
    # [pair, rec, r16, kb, kq, 32 codes] -> bit stream of 192 bits per field, LSB first
    f = full.reshape(rp // 32, 2, 16, KB, 4, 32)
    bits = ((f[..., None] >> np.arange(6, dtype=np.uint8)) & 1).reshape(rp // 32, 2, 16, KB, 4, 192)
    by = np.packbits(bits, axis=-1, bitorder="little")       # [pair, rec, r16, kb, kq, 24]
    by = by.transpose(0, 3, 1, 4, 2, 5)                      # [pair, kb, rec, kq, r16, 24]: lane = r16 + 16 kq
    out = np.zeros((rp // 32, KB, PAIR_BYTES), dtype=np.uint8)
    out[:, :, :2048] = by[..., :16].reshape(rp // 32, KB, 2048)
    out[:, :, 2048:] = by[..., 16:].reshape(rp // 32, KB, 1024)
    return out.reshape(-1)


def unpack(buf, rows, K, row_pad=32):
    """packed plane -> codes uint8 [rows, K] (the padding is returned by unpack_full)"""
    return unpack_full(buf, rows, K, row_pad)[:rows, :K]


def unpack_full(buf, rows, K, row_pad=32):
    rp, kp = -(-rows // row_pad) * row_pad, -(-K // 128) * 128
    KB = kp // 128
    b = np.asarray(buf, dtype=np.uint8)[: (rp // 32) * KB * PAIR_BYTES].reshape(rp // 32, KB, PAIR_BYTES)
    by = np.concatenate([b[:, :, :2048].reshape(rp // 32, KB, 2, 4, 16, 16), b[:, :, 2048:].reshape(rp // 32, KB, 2, 4, 16, 8)], axis=-1)
    bits = np.unpackbits(by, axis=-1, bitorder="little").reshape(rp // 32, KB, 2, 4, 16, 32, 6)
    codes = (bits.astype(np.uint8) << np.arange(6, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)   # [pair, kb, rec, kq, r16, 32]
    return codes.transpose(0, 2, 4, 1, 3, 5).reshape(rp, kp)


def digits_of(w):
    """integer w, |w| <= 2^24 -> five balanced radix-32 digits [..., 5], least significant first: sum d_i 32^i == w, |d_i| <= 16
    (digits of |w| with d in (-16, 16], the sign applied afterwards)"""
    w = np.asarray(w, dtype=np.int64)
    sgn = np.where(w < 0, -1, 1)
    a = np.abs(w)
    out = []
    for _ in range(NDIGITS):
        d = a & 31
        d = np.where(d > 16, d - 32, d)
        a = (a - d) >> 5
        out.append(sgn * d)
    if (a != 0).any():
        raise ValueError("integer does not fit five balanced radix-32 digits")
    return np.stack(out, axis=-1)


def from_digits(d):
    d = np.asarray(d, dtype=np.int64)
    return (d * (32 ** np.arange(NDIGITS, dtype=np.int64))).sum(axis=-1)


def row_exponent(wp):
    """W' float64 [N, K] -> E int [N] with 2^23 <= max_k |W'[n,k]| 2^E[n] < 2^24; E = 0 for an all-zero row"""
    mx = np.abs(np.asarray(wp, dtype=np.float64)).max(axis=1)
    _, ex = np.frexp(mx)                                     # mx = f 2^ex, f in [0.5, 1)
    return np.where(mx > 0, 24 - ex, 0).astype(np.int64)


def weight_integers(wp, E=None):
    """w = rint(W' 2^E[n]) in float64 (ties to even), int64 [N, K]"""
    wp = np.asarray(wp, dtype=np.float64)
    E = row_exponent(wp) if E is None else E
    return np.rint(np.ldexp(wp, E[:, None].astype(np.int64))).astype(np.int64)


def pack_weight(wp, row_pad=128):
    """W' [N, K] -> (five packed planes [5, bytes], E [N])"""
    E = row_exponent(wp)
    d = digits_of(weight_integers(wp, E))
    return np.stack([pack(encode_digit(d[..., i]), row_pad) for i in range(NDIGITS)]), E


def unpack_weight(planes, N, K, row_pad=128):
    """five packed planes -> w int64 [N, K]"""
    d = np.stack([np.rint(e2m3_decode(unpack(planes[i], N, K, row_pad)) * 8.0).astype(np.int64) for i in range(NDIGITS)], axis=-1)
    return from_digits(d)
