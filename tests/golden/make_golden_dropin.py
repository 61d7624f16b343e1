#!/usr/bin/env python3
"""Golden fixtures for the drop-in tests (tests/test_dropin_reference_model.py, tests/test_dropin_reference_cpt.py): the
reference's own model assemblies in the small configurations of those tests, built with seed 0 on the reference's own classes.

  dropin_sp.npz   part1 models_sp.SPLMHeadModel (2 layers, n_embd 32, widths 4/6/32): the state dict (key order, shapes,
                  values), seeded token ids and the 32-bit logits of the model on them.
  dropin_cpt.npz  part2 cpt_model.CPTModel (2 layers, n_embd 32, widths 4/6/32): the state dict, and for every CPTLinear its
                  constructor arguments, a seeded input and its 32-bit output.

Run on a machine with a checkout of the reference (CPU, fp32):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dropin.py <reference checkout>
Outputs are data only."""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
torch.set_grad_enabled(False)

SP_CONFIG = dict(vocab_size=97, n_positions=32, n_embd=32, n_layer=2, n_head=4)
SP_EXTRA = dict(bit_widths=[4, 6, 32], lora_rank_per_bit={4: 4, 6: 4, 32: 0}, lora_alpha_per_bit={4: 4, 6: 4, 32: 0},
                quantizer_per_bit={4: "minmax", 6: "log", 32: None}, activation_bits_per_bit={4: 4, 6: 6, 32: 32},
                per_channel_quantization=True, layer_norm_epsilon=1e-5, embd_pdrop=0.0)
CPT_CONFIG = dict(vocab_size=97, n_positions=32, n_embd=32, n_layer=2, n_head=4, layer_norm_epsilon=1e-5, embd_pdrop=0.0,
                  bit_widths=[4, 6, 32], shared_lora_rank=4, shared_lora_alpha=8,
                  quantizer_per_bit={4: "log", 6: "log", 32: None}, gradient_bits=8)


def _state(sd):
    keys = list(sd.keys())
    return keys, {f"p{i}": sd[k].detach().cpu().numpy() for i, k in enumerate(keys)}


def make_sp(ref):
    from transformers import GPT2Config
    sys.path.insert(0, ref)
    models = importlib.import_module("part1_switchable_precision.models_sp")
    cfg = GPT2Config(**SP_CONFIG)
    for k, v in SP_EXTRA.items():
        setattr(cfg, k, v)
    torch.manual_seed(0)
    model = models.SPLMHeadModel(cfg)
    model.set_precision(32)
    model.eval()
    ids = torch.randint(0, SP_CONFIG["vocab_size"], (2, 16), generator=torch.Generator().manual_seed(1))
    out = model(ids)
    logits = out if torch.is_tensor(out) else (out["logits"] if isinstance(out, dict) else out.logits)
    keys, arrays = _state(model.state_dict())
    meta = {"keys": keys, "config": SP_CONFIG, "extra": {k: (v if not isinstance(v, dict) else {str(b): x for b, x in v.items()})
                                                         for k, v in SP_EXTRA.items()}}
    np.savez(os.path.join(HERE, "dropin_sp.npz"), meta=np.array(json.dumps(meta)), ids=ids.numpy(),
             logits=logits.numpy(), **arrays)


def make_cpt(ref):
    part2 = os.path.join(ref, "part2_cyclic_precision_training")
    sys.path.insert(0, part2)          # the reference imports its siblings by bare name
    cm = importlib.import_module("cpt_model")
    cfg = {"model": types.SimpleNamespace(**CPT_CONFIG), "training": types.SimpleNamespace(target_bits=6)}
    torch.manual_seed(0)
    model = cm.CPTModel(cfg)
    model.set_precision(32)
    model.eval()
    gen = torch.Generator().manual_seed(2)
    layers, io = [], {}
    for name, m in model.named_modules():
        if isinstance(m, cm.CPTLinear):
            i = len(layers)
            layers.append({"name": name, "in": m.in_features, "out": m.out_features, "bias": m.linear.bias is not None})
            x = torch.randn(2, 16, m.in_features, generator=gen)
            io[f"x{i}"], io[f"y{i}"] = x.numpy(), m(x).numpy()
    keys, arrays = _state(model.state_dict())
    meta = {"keys": keys, "layers": layers,
            "config": {k: (v if not isinstance(v, dict) else {str(b): x for b, x in v.items()}) for k, v in CPT_CONFIG.items()}}
    np.savez(os.path.join(HERE, "dropin_cpt.npz"), meta=np.array(json.dumps(meta)), **io, **arrays)


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "part1_switchable_precision")):
        sys.exit("usage: make_golden_dropin.py <reference checkout>")
    make_sp(os.path.abspath(sys.argv[1]))
    make_cpt(os.path.abspath(sys.argv[1]))
