"""CPU: the drop-in claim itself, against the reference's own GPT-2 assembly (part1_switchable_precision/models_sp.py) as
recorded in tests/golden/dropin_sp.npz (tests/golden/make_golden_dropin.py: the reference's SPLMHeadModel built with seed 0,
its state dict, seeded token ids and its 32-bit logits).  This build's model on the drop-in classes must expose the same
state dict, load the reference's checkpoint strictly, fan out set_precision() and toggle calibration_mode exactly as the
reference's model does, and give the reference's 32-bit logits.  No quantized compute (no GPU here)."""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from helpers import assert_close_y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fixture():
    z = np.load(os.path.join(GOLDEN, "dropin_sp.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    sd = OrderedDict((k, torch.from_numpy(z[f"p{i}"])) for i, k in enumerate(meta["keys"]))
    return meta, sd, torch.from_numpy(z["ids"]), torch.from_numpy(z["logits"])


def _config(meta):
    from transformers import GPT2Config
    cfg = GPT2Config(**meta["config"])
    for k, v in meta["extra"].items():
        setattr(cfg, k, {int(b): x for b, x in v.items()} if isinstance(v, dict) else v)
    return cfg


def _build(meta):
    import llm_qat_on_gpt2_amd as pkg
    torch.manual_seed(0)
    return pkg.SPLMHeadModel(_config(meta))


def _logits(o):
    return o if torch.is_tensor(o) else (o["logits"] if isinstance(o, dict) else o.logits)


def test_reference_model_builds_on_the_dropin_layers():
    import llm_qat_on_gpt2_amd as pkg
    meta, sd_ref, ids, logits_ref = _fixture()
    mine = _build(meta)
    layers = [m for m in mine.modules() if m.__class__.__name__ == "SPLinearWithLoRA"]
    assert len(layers) == 8 and all(isinstance(m, pkg.SPLinearWithLoRA) for m in layers)      # 4 per block x 2 blocks
    sd_mine = mine.state_dict()
    assert list(sd_ref.keys()) == list(sd_mine.keys())
    assert {k: tuple(v.shape) for k, v in sd_ref.items()} == {k: tuple(v.shape) for k, v in sd_mine.items()}
    mine.load_state_dict(sd_ref, strict=True)                                               # reference checkpoint loads
    # set_precision fan-out (models_sp.py:224-234, 147-152, 52-56, 116-122)
    assert mine.set_precision(4) == 4 and all(m.current_bits == 4 for m in layers)
    with pytest.raises(ValueError):
        mine.set_precision(5)
    mine.set_precision(32)
    assert all(m.current_bits == 32 for m in layers)
    # calibration toggles match on the class NAME (models_sp.py:236-246)
    mine.disable_lora_for_calibration()
    assert all(m.calibration_mode for m in layers)
    mine.enable_lora_after_calibration()
    assert not any(m.calibration_mode for m in layers)
    # the teacher path (32 bit) is plain F.linear and runs anywhere: the reference model's logits with the same weights
    mine.eval()
    with torch.no_grad():
        lm = _logits(mine(ids))
    assert_close_y(lm, logits_ref, "32-bit logits")                 # the project's parity bound: recorded on another host's CPU
    # below 32 bits the layers are HIP-only: a CPU tensor is refused loudly instead of silently falling back
    mine.set_precision(4)
    for m in layers:
        for q in (m.quantizers_weight["4bit"], m.quantizers_input["4bit"]):
            q.calibrated = True
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        mine(ids)


def test_reference_model_builds_on_the_dropin_block_pieces():
    """The same with SwitchableLayerNorm and SPMLP: identical state dict, reference checkpoint loads, the reference's 32-bit
    logits (the teacher path is plain torch)."""
    import llm_qat_on_gpt2_amd as pkg
    meta, sd_ref, ids, logits_ref = _fixture()
    mine = _build(meta)
    assert sum(isinstance(m, pkg.SwitchableLayerNorm) for m in mine.modules()) == 2 * 2 + 1
    assert sum(isinstance(m, pkg.SPMLP) for m in mine.modules()) == 2
    sd_mine = mine.state_dict()
    assert list(sd_ref.keys()) == list(sd_mine.keys())
    mine.load_state_dict(sd_ref, strict=True)
    assert mine.set_precision(4) == 4
    assert all(m.current_precision == 4 for m in mine.modules() if isinstance(m, pkg.SwitchableLayerNorm))
    mine.set_precision(32); mine.eval()
    with torch.no_grad():
        lm = _logits(mine(ids))
    assert_close_y(lm, logits_ref, "32-bit logits")                 # the project's parity bound: recorded on another host's CPU
