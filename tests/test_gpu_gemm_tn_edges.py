"""GPU: spq_gemm_f32_tn (the token contraction of d/dA, d/dB and d/dW) at every launch edge, bit-exact.

Operands are integers in -3..3 held as fp32 and alpha is 1, 0.5 or -2: every partial sum is an integer below 9 * 16385 < 2^24,
so every summation order gives the same fp32 and the comparison is ``torch.equal`` against an integer reference -- a dropped,
doubled or misplaced token or column is a wrong integer, and there is no tolerance to argue about.  (The reference is held as
int64; the sum itself runs as a float64 matmul, which is exact on integers this small.)

The cases (tests/linear_grad_ref.py: TN_SHAPES x TN_LAYOUTS; their coverage of the planner is asserted, without a GPU, in
test_linear_grad_ref_cpu.py) go through the C ABI, because only there can the leading dimensions and the base pointers be set:
pitches longer than the row, even and odd, ldq % 4 in {0, 1, 2}, and operands one float past a 16-byte boundary.  The output has
64 floats behind it, the workspace 256 bytes behind the size the library asked for; everything is pre-filled -- the output and
the partial sums with NaN, so an element nobody wrote fails the comparison -- and the guards must come back untouched."""
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


def _operand(rows, cols, ld, off, gen, integer=True):
    """[rows, cols] view with row pitch ld, starting ``off`` floats into a 16-byte aligned buffer; the padding holds NaN (a
    kernel that reads it into a sum shows)"""
    flat = torch.full((off + rows * ld + 8,), float("nan"), device=DEV)
    assert flat.data_ptr() % 16 == 0
    v = torch.as_strided(flat, (rows, cols), (ld, 1), off)
    if integer:
        v.copy_(torch.randint(-3, 4, (rows, cols), generator=gen, device=DEV).float())
    else:
        v.copy_(torch.randn(rows, cols, generator=gen, device=DEV))
    assert v.data_ptr() == flat.data_ptr() + 4 * off
    return flat, v


def _call_tn(pkg, p, ldp, q, ldq, M, I, J, alpha):
    """the raw C call with guarded output and workspace; returns out [I, J]"""
    lib = pkg._lib.load()
    nbytes = lib.spq_gemm_f32_tn_workspace_bytes(M, I, J)
    ws = torch.full((nbytes + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    ws[:nbytes - nbytes % 4].view(torch.float32).fill_(float("nan"))
    buf = torch.full((I * J + 64,), GUARD, device=DEV)
    buf[:I * J].fill_(float("nan"))
    rc = lib.spq_gemm_f32_tn(p.data_ptr(), ldp, q.data_ptr(), ldq, M, I, J, float(alpha), buf.data_ptr(), ws.data_ptr(), nbytes,
                             pkg._lib.stream_ptr(torch.device(DEV)))
    pkg._lib.check(rc, "spq_gemm_f32_tn")
    torch.cuda.synchronize()
    assert bool((buf[I * J:] == GUARD).all()), "the 64 floats behind the output were written"
    assert bool((ws[nbytes:] == 0xA5).all()), "the 256 bytes behind the workspace were written"
    return buf[:I * J].view(I, J)


@pytest.mark.parametrize("M,I,J,layout,alpha", R.tn_cases(), ids=lambda v: str(v))
def test_tn_is_the_integer_sum(pkg, M, I, J, layout, alpha):
    ldp, ldq, offp, offq = R.tn_leading_dims(I, J, layout)
    gen = torch.Generator(device=DEV).manual_seed(M * 7 + I * 3 + J)
    _, p = _operand(M, I, ldp, offp, gen)
    _, q = _operand(M, J, ldq, offq, gen)
    want = (p.double().t() @ q.double()).round().to(torch.int64)                 # exact: |sum| <= 9 M < 2^24
    assert int(want.abs().max()) < 2 ** 24
    out = _call_tn(pkg, p, ldp, q, ldq, M, I, J, alpha)
    ref = (want.double() * alpha).float()
    if not torch.equal(out, ref):
        bad = (out != ref) | out.isnan()
        ij = bad.nonzero()[0].tolist()
        raise AssertionError(f"tn({M},{I},{J}) {layout} alpha={alpha} plan={R.tn_plan(pkg._lib.load(), M, I, J)}: {int(bad.sum())} of {I * J} "
                             f"elements wrong, first at {ij}: got {float(out[ij[0], ij[1]])}, want {float(ref[ij[0], ij[1]])}")


@pytest.mark.parametrize("M,I,J", [(65, 64, 128), (257, 66, 128), (2305, 130, 130), (16385, 8, 8)])     # S = 1, 3, 19, 128
def test_tn_two_runs_are_bit_identical(pkg, M, I, J):
    """random fp32 operands, where the order of summation shows: the split over tokens is reduced in a fixed order"""
    gen = torch.Generator(device=DEV).manual_seed(M)
    _, p = _operand(M, I, I, 0, gen, integer=False)
    _, q = _operand(M, J, J, 0, gen, integer=False)
    a = _call_tn(pkg, p, I, q, J, M, I, J, 0.5).clone()
    b = _call_tn(pkg, p, I, q, J, M, I, J, 0.5)
    assert torch.equal(a, b)
    assert R.worst_ratio(a, 0.5 * (p.double().t() @ q.double())) <= 1.0


def test_gemm_tn_swap_branch(pkg):
    """_gemm_tn puts the thin operand on the left (I > J: computes Q^T . P and transposes); same integers either way"""
    from llm_qat_on_gpt2_amd.sp_linear import _gemm_tn
    M, I, J = 300, 200, 16
    gen = torch.Generator(device=DEV).manual_seed(5)
    p = torch.randint(-3, 4, (M, I), generator=gen, device=DEV).float()
    q = torch.randint(-3, 4, (M, J), generator=gen, device=DEV).float()
    swapped = _gemm_tn(p, q, -2.0)
    direct = _call_tn(pkg, p, I, q, J, M, I, J, -2.0)
    assert swapped.shape == (I, J) and swapped.is_contiguous()
    assert torch.equal(swapped, direct)
    assert torch.equal(swapped, _gemm_tn(q, p, -2.0).t())
    assert torch.equal(direct.double(), -2.0 * (p.double().t() @ q.double()))
