#!/usr/bin/env python3
"""Golden fixtures for SwitchableLayerNorm under autograd: the reference's own SwitchableLayerNorm (imported from
/root/reference, CPU, fp32) run forward and backward on seeded inputs.  Stored per case: x, g, weight, bias, y, dx, dweight,
dbias (data only) and, in the meta, the reference's own err/bound against the same formula in fp64 -- the figure that decides
whether the fp32 reference or fp64 is the yardstick for that case (tests/ln_grad_ref.py:yardstick).

Asserts on the way that oracle.ref_cpu.switchable_layernorm under torch's autograd equals the reference bit for bit, so tests at
larger shapes can use the oracle.

Run in the build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lngrad.py
Outputs: tests/golden/lngrad_*.npz."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
sys.dont_write_bytecode = True

from part1_switchable_precision.switchable_batchnorm import SwitchableLayerNorm  # noqa: E402  (the reference)

import ln_grad_ref as R  # noqa: E402


def case(name, rows_shape, C, seed, dist="normal", offset=None):
    rows = int(np.prod(rows_shape))
    x, g, w, b = R.make_case(dist, rows, C, seed)
    if offset is not None:                                    # rows with a large common offset: 0.1 randn + offset
        x = x * 0.1 + offset
    x, g = x.reshape(*rows_shape, C), g.reshape(*rows_shape, C)
    ln = SwitchableLayerNorm(C, precision_levels=[4, 32], eps=1e-5)
    ln.set_precision(4)
    ln.weights["4"].data = w.clone()
    ln.biases["4"].data = b.clone()
    xs = x.clone().requires_grad_(True)
    y = ln(xs)
    y.backward(g)
    ref = (xs.grad, ln.weights["4"].grad, ln.biases["4"].grad)
    yo, *oracle = R.oracle_grads(x, g, w, b, 1e-5, torch.float32)
    assert torch.equal(y.detach(), yo), f"{name}: oracle forward != reference"
    for a, o, what in zip(ref, oracle, ("dx", "dweight", "dbias")):
        assert torch.equal(a, o), f"{name}: oracle {what} != reference"
    _, limit, ratio, which = R.yardstick(x, g, w, b, 1e-5)
    meta = {"name": name, "C": C, "dist": dist, "offset": offset, "seed": seed, "ref_ratio_vs_fp64": ratio, "yardstick": which}
    out = {"x": x, "g": g, "weight": w, "bias": b, "y": y.detach(), "dx": ref[0], "dweight": ref[1], "dbias": ref[2]}
    path = os.path.join(HERE, f"lngrad_{name}.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **{k: v.numpy() for k, v in out.items()})
    print(f"  lngrad {name}: fp32 reference at {ratio:.3f} of the bar against fp64 -> yardstick {which}; {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    case("768", (2, 40), 768, 11)
    case("1024", (21,), 1024, 12)
    case("64", (5,), 64, 13)
    case("768_channel", (48,), 768, 14, dist="channel")
    case("768_offset", (40,), 768, 15, offset=5.0)
