"""CPU: part2's own model assembly (part2_cyclic_precision_training/cpt_model.py: CPTModel -> CPTBlock -> CPTSelfAttention /
CPTLinear) as recorded in tests/golden/dropin_cpt.npz (tests/golden/make_golden_dropin.py: the reference's CPTModel built with
seed 0, its state dict, and every CPTLinear's constructor arguments with a seeded input and its 32-bit output).  Every one of
its CPTLinear layers, rebuilt as this build's CPTLinear with the same arguments -- the one-name swap of INTEGRATION.md -- must
hold the same state-dict entries, load the reference's strictly, fan out set_precision() and give the reference layer's
32-bit output.  No quantized compute (no GPU here)."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import assert_close_y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_reference_cpt_model_builds_on_the_dropin_layer():
    import llm_qat_on_gpt2_amd as pkg
    z = np.load(os.path.join(GOLDEN, "dropin_cpt.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    cfg = meta["config"]
    sd_ref = {k: torch.from_numpy(z[f"p{i}"]) for i, k in enumerate(meta["keys"])}
    layers = meta["layers"]
    assert len(layers) == 2 * 4 + 1                                                 # 4 per block + lm_head
    covered = set()
    for i, lay in enumerate(layers):
        m = pkg.cpt.CPTLinear(lay["in"], lay["out"], cfg["bit_widths"], {int(b): q for b, q in cfg["quantizer_per_bit"].items()},
                              cfg["gradient_bits"], bias=lay["bias"], shared_lora_rank=cfg["shared_lora_rank"],
                              shared_lora_alpha=cfg["shared_lora_alpha"])
        assert m.__class__.__name__ == "CPTLinear"             # what the reference's calibration toggles match on
        pre = lay["name"] + "."
        ref_keys = [k for k in meta["keys"] if k.startswith(pre)]
        sd_mine = m.state_dict()
        assert ref_keys == [pre + k for k in sd_mine.keys()], lay["name"]
        assert {k: tuple(sd_ref[k].shape) for k in ref_keys} == {pre + k: tuple(v.shape) for k, v in sd_mine.items()}, lay["name"]
        m.load_state_dict({k[len(pre):]: sd_ref[k] for k in ref_keys}, strict=True)
        covered.update(ref_keys)
        m.set_precision(4)
        assert m.current_bits == 4 and m.quantizer_input.num_bits == 4
        with pytest.raises(ValueError):
            m.set_precision(5)
        # the 32-bit path is plain F.linear and runs anywhere: the reference layer's output with the same weights
        m.set_precision(32); m.eval()
        with torch.no_grad():
            y = m(torch.from_numpy(z[f"x{i}"]))
        assert_close_y(y, torch.from_numpy(z[f"y{i}"]), lay["name"])      # the project's parity bound: recorded on another host's CPU
    # everything else in the reference's state dict belongs to the assembly itself (embeddings, LayerNorms)
    rest = [k for k in meta["keys"] if k not in covered]
    assert rest == ["wte.weight", "wpe.weight"] + [f"h.{b}.{ln}.{p}" for b in range(2) for ln in ("ln_1", "ln_2") for p in ("weight", "bias")] \
        + ["ln_f.weight", "ln_f.bias"], rest
