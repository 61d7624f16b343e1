"""GPU: spq_gemm_f32_nt (g . FQ(B)^T, the two-segment d/dx and the rank-r weight update of the backward) at every edge, bit-exact.

Integer operands in -3..3 as fp32, K <= 1024, alpha2 in {1, 0.5} (1 skips the kernel's scaling branch), an integer bias or none:
every partial sum is a multiple of 0.5 far below 2^23, so the result does not depend on the summation order and the
comparison is ``torch.equal`` against the exact integer sum (a float64 matmul, exact on integers this small).

The cases come from tests/linear_grad_ref.py (nt_cases; test_linear_grad_ref_cpu.py asserts, without a GPU, which branch each one
reaches): K = 1 ... 100 with tight and padded pitches in both kernel instantiations -- the scalar-load one forced once by an odd
pitch and once by a base pointer one float past a 16-byte boundary --, M and N around the 128 tile, the second segment at
K2 = 0 ... 129, and workgroup counts 1 ... 17 for the XCD remap of the workgroup index.  C is written into a sentinel-filled
buffer, once with ldc = N and once with ldc = N + 5, whose pad columns and tail must come back untouched."""
import pytest
import torch

import linear_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = -777.0


@pytest.fixture(scope="module")
def pkg():
    import llm_qat_on_gpt2_amd as p
    p._lib.load()
    return p


def _operand(rows, cols, ld, off, gen):
    flat = torch.full((off + rows * ld + 8,), float("nan"), device=DEV)          # NaN padding: reading it into a sum shows
    assert flat.data_ptr() % 16 == 0
    v = torch.as_strided(flat, (rows, cols), (ld, 1), off)
    v.copy_(torch.randint(-3, 4, (rows, cols), generator=gen, device=DEV).float())
    return v


@pytest.mark.parametrize("case", R.nt_cases(), ids=lambda c: c["tag"])
def test_nt_is_the_integer_sum(pkg, case):
    c = case
    M, N, K, K2 = c["M"], c["N"], c["K"], c["K2"]
    gen = torch.Generator(device=DEV).manual_seed(M + 3 * N + 5 * K + 7 * K2)
    A = _operand(M, K, c["lda"], c["offa"], gen)
    B = _operand(N, K, c["ldb"], c["offb"], gen)
    A2 = _operand(M, K2, c["lda2"], c["offa2"], gen) if K2 else None
    B2 = _operand(N, K2, c["ldb2"], c["offb2"], gen) if K2 else None
    bias = torch.randint(-3, 4, (N,), generator=gen, device=DEV).float() if c["bias"] else None
    want = A.double() @ B.double().t()
    if K2:
        want = want + c["alpha2"] * (A2.double() @ B2.double().t())
    if bias is not None:
        want = want + bias.double()
    assert float(want.abs().max()) < 2 ** 22 and torch.equal(want * 2, (want * 2).round())
    want = want.float()
    lib = pkg._lib.load()
    ptr = pkg._lib.ptr
    for ldc in (N, N + 5):
        buf = torch.full((M * ldc + 64,), GUARD, device=DEV)
        Cv = torch.as_strided(buf, (M, N), (ldc, 1), 0)
        Cv.fill_(float("nan"))                                                   # an element nobody writes fails the comparison
        rc = lib.spq_gemm_f32_nt(A.data_ptr(), c["lda"], B.data_ptr(), c["ldb"], K, ptr(A2), c["lda2"] if K2 else 0, ptr(B2),
                                 c["ldb2"] if K2 else 0, K2, c["alpha2"], ptr(bias), buf.data_ptr(), ldc, M, N,
                                 pkg._lib.stream_ptr(torch.device(DEV)))
        pkg._lib.check(rc, "spq_gemm_f32_nt")
        torch.cuda.synchronize()
        if not torch.equal(Cv, want):
            bad = (Cv != want) | Cv.isnan()
            ij = bad.nonzero()[0].tolist()
            raise AssertionError(f"nt {c['tag']} (fast={R.nt_fast(c)}, ldc={ldc}): {int(bad.sum())} of {M * N} elements wrong, first at {ij}: "
                                 f"got {float(Cv[ij[0], ij[1]])}, want {float(want[ij[0], ij[1]])}")
        guard = torch.ones(M * ldc + 64, dtype=torch.bool, device=DEV)
        torch.as_strided(guard, (M, N), (ldc, 1), 0).fill_(False)
        assert bool((buf[guard] == GUARD).all()), f"nt {c['tag']} ldc={ldc}: pad columns or the tail behind C were written"
