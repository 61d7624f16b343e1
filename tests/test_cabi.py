"""CPU: the C-ABI shared library loads and exports every symbol include/spq.h declares (no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import llm_qat_on_gpt2_amd as pkg
    if not os.path.exists(pkg._lib.LIB_PATH):
        g.build()
    return pkg._lib.load()


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "spq.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(spq_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(lib):
    import llm_qat_on_gpt2_amd as pkg
    names = declared_symbols()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/spq.h but not exported by libspq.so"
        assert n in pkg._lib.SIGNATURES, f"{n} has no ctypes signature in _lib.py"
    assert sorted(pkg._lib.SIGNATURES) == names


def test_version_and_error_string(lib):
    assert lib.spq_version() == 101
    assert isinstance(lib.spq_last_error(), bytes)


def test_argument_validation_without_gpu(lib):
    """Pure host-side argument checks: rejected before any HIP call."""
    import llm_qat_on_gpt2_amd as pkg
    rc = lib.spq_finish_scale(None, None, 4, 8, 0, 1, 1e-5, None, None, None)
    assert rc == -1 and b"null pointer" in lib.spq_last_error()
    rc = lib.spq_fakequant(None, 1, 1, 1, None, None, 0, 8, 0, 1, None, None, 0, None)
    assert rc == -1
    assert lib.spq_fwd_workspace_bytes(0, 1, 1, 0, pkg._lib.PATH_F32) == 0
    assert lib.spq_fwd_workspace_bytes(128, 64, 64, 8, pkg._lib.PATH_F32) >= 128 * 64 * 4 + 128 * 8 * 4
    assert lib.spq_stats_workspace_bytes(8192, 768, 1, 1) > 0
    with pytest.raises(pkg._lib.SpqError):
        pkg._lib.check(rc, "spq_fakequant")


def test_struct_layout_matches_header(tmp_path):
    """sizeof / offsetof of both argument structs as gcc lays include/spq.h out, against the ctypes mirrors."""
    import subprocess
    import llm_qat_on_gpt2_amd as pkg
    structs = {"spq_fwd_args": pkg._lib.FwdArgs, "spq_prepare_args": pkg._lib.PrepareArgs}
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "spq.h")}"', 'int main(void) {']
    for cname, st in structs.items():
        src.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for fname, _ in st._fields_:
            src.append(f'  printf("{cname}.{fname} %zu\\n", offsetof({cname}, {fname}));')
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", str(c), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, st in structs.items():
        assert int(out[cname]) == ctypes.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(out[f"{cname}.{fname}"]) == getattr(st, fname).offset, f"{cname}.{fname}"


def _made_up_fwd_args(pkg, keep, **kw):
    """F16X2, M=256 K=128 N=128 r=16, 4-bit symmetric minmax, every operand a made-up 16-byte-aligned address (nothing on the
    host dereferences one) and a workspace said to be large.  `keep` holds the ctypes objects the struct points at."""
    L = pkg._lib
    fake = iter(range(0x7000_0000_0000, 0x7100_0000_0000, 0x1000_0000))
    a = L.FwdArgs(M=256, K=128, N=128, r=16, bits=4, qtype=0, symmetric=1, quantize_input=1, x_per_channel=1, path=L.PATH_F16X2,
                  lora_scaling=1.0, workspace_bytes=1 << 40, ln_eps=1e-5)
    for f in ("x", "sx", "zx", "w_prep", "w_rowscale", "bias", "a_prep", "b_prep", "y", "workspace"):
        setattr(a, f, next(fake))
    with_prepare = kw.pop("with_prepare", False)
    for k, v in kw.items():
        setattr(a, k, next(fake) if v == "ptr" else v)
    if with_prepare:                                           # a filled spq_prepare_args for the same layer
        q = L.PrepareArgs(N=a.N, K=a.K, r=a.r, w_per_channel=1, w_bits=4, w_symmetric=1, b_per_channel=1, b_bits=4, b_symmetric=1,
                          scaling=1.0, a_per_channel=0, a_bits=4, a_symmetric=1, x_per_channel=a.x_per_channel, path=a.path,
                          w_prep=a.w_prep, w_prep_bytes=L.load().spq_prep_bytes(a.N, a.K, a.r, a.path), w_rowscale=a.w_rowscale,
                          a_prep=a.a_prep, sx=a.sx)
        for f in ("W", "sw", "zw", "B", "sb", "zb", "A", "sa", "za"):
            setattr(q, f, next(fake))
        keep.append(q)
        a.prepare = ctypes.pointer(q)
    return a


@pytest.mark.parametrize("kw,code,word", [
    # refused only after the activation pass (or the weight preparation) had been enqueued, before validate / plan / launch were split
    (dict(epilogue=1, N=130), -3, b"the fused GELU / levels-out epilogues need N % 4 == 0"),
    (dict(out_levels="ptr", out_scale="ptr", out_levels_ld=128, out_bits=13), -3, b"levels-out store needs"),
    (dict(K=2048, ln_weight="ptr", ln_bias="ptr", with_prepare=True), -3, b"the LayerNorm prologue needs"),
    # refused first all along: same code, same text
    (dict(bits=13), -3, b"SPQ_PATH_F16X2 needs a symmetric minmax input quantizer with 2..12 bits"),
    (dict(path=5, x_per_channel=1), -3, b"SPQ_PATH_I8 needs a per-tensor input scale"),
    (dict(path=3), -3, b"SPQ_PATH_U8X2 (byte-level ring kernel)"),
    (dict(a_limb_scale="ptr"), -3, b"a_limb_scale (LoRA-down on the f16 pipe"),
    (dict(K=2048, ln_weight="ptr", ln_bias="ptr"), -3, b"the LayerNorm prologue needs"),
    (dict(stage=2, with_prepare=True), -1, b"prepare args go with the activation stage"),
])
def test_forward_refusals_precede_every_launch(lib, kw, code, word):
    """Every refusal of the fused forward is decided before anything is enqueued: without a device a launch attempt would show as
    SPQ_ERR_LAUNCH (-2) instead of the refusal.  The operand addresses are made up, so this must never run where a kernel could
    be reached."""
    import torch
    import llm_qat_on_gpt2_amd as pkg
    if torch.cuda.is_available():
        pytest.skip("made-up operand addresses: only where no launch can succeed")
    keep = []
    rc = lib.spq_linear_lora_fwd(ctypes.byref(_made_up_fwd_args(pkg, keep, **dict(kw))), None)
    assert rc == code, (rc, lib.spq_last_error())
    assert word in lib.spq_last_error(), lib.spq_last_error()
