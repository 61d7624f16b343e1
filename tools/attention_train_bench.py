"""The causal attention core under a gradient: the HIP forward / backward pair (set_attention_core(..., 'hip', backward=True))
against torch's fused SDPA and the reference's explicit formula, in ONE process, the variants alternated `--repeats` times,
HIP-event timing.

(a) SPAttention.core alone, forward + backward, at 8 x 12 x 1024 x 64 and 32 x 12 x 1024 x 64 -- plus the library's kernels alone
    through the C ABI (forward with lse; the three backward launches), with the causal FLOP count of the backward's seven tile
    products as a fraction of the fp32 matrix peak;
(b) one SPBlock and the 12-layer SPModel, training step (forward + backward), 8 x 1024 tokens, 4-bit min-max + LoRA r = 64, base
    weights frozen, hip+backward against SDPA, with torch.cuda.max_memory_allocated.
Prints one JSON document; --out writes it to a file."""
import argparse
import json
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import llm_qat_on_gpt2_amd as pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--iters', type=int, default=10)
ap.add_argument('--layers', type=int, default=12)
ap.add_argument('--out', default=None)
args = ap.parse_args()
dev = torch.device('cuda:0')
F32_MATRIX_PEAK = 157.3e12
E, H, D, T, bits, r = 768, 12, 64, 1024, 4, 64


def time_ms(fn, iters, warm=3):
    """mean of `iters` back-to-back calls between two HIP events, after `warm` untimed calls"""
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def summary(v):
    return {'median': statistics.median(v), 'min': min(v), 'max': max(v), 'runs': v}


def alternate(step, module, variants):
    """{variant: summary}: the variants alternated args.repeats times, peak memory of the last repeat"""
    times, mem = {v: [] for v in variants}, {}
    for _ in range(args.repeats):
        for v in variants:
            pkg.set_attention_core(module, 'hip' if v == 'hip_backward' else v, backward=v == 'hip_backward')
            torch.cuda.reset_peak_memory_stats()
            times[v].append(time_ms(step, args.iters))
            mem[v] = torch.cuda.max_memory_allocated()
    pkg.set_attention_core(module, 'sdpa')
    out = {v: dict(summary(times[v]), peak_bytes=mem[v]) for v in variants}
    for v in variants:
        if v != 'hip_backward':
            out[f'{v}_over_hip_backward'] = out[v]['median'] / out['hip_backward']['median']
    return out


cfg = types.SimpleNamespace(vocab_size=1024, n_positions=T, n_embd=E, n_layer=args.layers, n_head=H, layer_norm_epsilon=1e-5,
                            bit_widths=[bits, 32], lora_rank_per_bit={bits: r, 32: 0}, lora_alpha_per_bit={bits: 64, 32: 0},
                            quantizer_per_bit={bits: 'minmax', 32: None}, per_channel_quantization=True)
result = {'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'iters': args.iters, 'unit': 'ms'}

# ---- (a) the core alone ---------------------------------------------------------------------------------------------------------
lib = pkg._lib.load()
att = pkg.SPAttention(cfg, [bits, 32]).to(dev)
for B in (8, 32):
    gen = torch.Generator().manual_seed(B)
    qkv = torch.randn(B, T, 3 * E, generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(B, T, E, generator=gen).to(dev)

    def step():
        qkv.grad = None
        att.core(qkv).backward(g)
    entry = alternate(step, att, ('hip_backward', 'sdpa', 'explicit'))
    # the kernels alone, through the C ABI (no autograd, no allocation)
    x = qkv.detach()
    out, lse = pkg.causal_attention(x, H, return_lse=True)
    dqkv = torch.empty_like(x)
    ws = torch.empty(lib.spq_causal_attention_bwd_workspace_bytes(B, T, H, D), dtype=torch.uint8, device=dev)
    st = pkg._lib.stream_ptr(dev)
    fwd = lambda: lib.spq_causal_attention_fwd(x.data_ptr(), B, T, H, D, out.data_ptr(), lse.data_ptr(), st)
    bwd = lambda: lib.spq_causal_attention_bwd(x.data_ptr(), out.data_ptr(), lse.data_ptr(), g.data_ptr(), B, T, H, D,
                                               dqkv.data_ptr(), ws.data_ptr(), ws.numel(), st)
    assert fwd() == 0 and bwd() == 0
    kf = [time_ms(fwd, 20) for _ in range(args.repeats)]
    kb = [time_ms(bwd, 20) for _ in range(args.repeats)]
    pair_flop = 2 * D * B * H * T * (T + 1) / 2          # one q.k (or p.v) product over the causal pairs
    entry['kernel_forward'] = dict(summary(kf), flop=2 * pair_flop,
                                   fraction_of_f32_matrix_peak=2 * pair_flop / (statistics.median(kf) * 1e-3) / F32_MATRIX_PEAK)
    entry['kernel_backward'] = dict(summary(kb), flop=7 * pair_flop,
                                    fraction_of_f32_matrix_peak=7 * pair_flop / (statistics.median(kb) * 1e-3) / F32_MATRIX_PEAK)
    result[f'core_{B}x{H}x{T}x{D}'] = entry
    del qkv, g, x, out, lse, dqkv, ws

# ---- (b) one SPBlock and the SPModel, training step ---------------------------------------------------------------------------------
B = 8


def prepare(model, batches):
    torch.manual_seed(0)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if 'lora_B' in n: p.normal_(0, 0.01)
            elif p.dim() > 1 and 'lora_A' not in n: p.normal_(0, 0.02)
    model = model.to(dev).eval()
    pkg.calibrate_model(model, bits, batches)
    model.train()
    for m in model.modules():
        if m.__class__.__name__ == 'SPLinearWithLoRA':                # base weights frozen (main_sp.py:83)
            for p in m.linear.parameters():
                p.requires_grad_(False)
    return model


gen = torch.Generator().manual_seed(7)
xb = torch.randn(B, T, E, generator=gen).to(dev)
gb = torch.randn(B, T, E, generator=gen).to(dev)
blk = prepare(pkg.SPBlock(cfg, bit_widths=[bits, 32]), [xb, torch.randn(B, T, E, generator=gen).to(dev)])
xg = xb.clone().requires_grad_(True)


def block_step():
    xg.grad = None
    blk.zero_grad(set_to_none=True)
    blk(xg).backward(gb)
result['spblock_8x1024'] = alternate(block_step, blk, ('hip_backward', 'sdpa'))
del blk

ids = torch.randint(0, cfg.vocab_size, (B, T), generator=gen).to(dev)
model = prepare(pkg.SPModel(cfg), [ids, torch.randint(0, cfg.vocab_size, (B, T), generator=gen).to(dev)])


def model_step():
    model.zero_grad(set_to_none=True)
    model(ids).backward(gb)
result[f'spmodel_{args.layers}layer_8x1024'] = alternate(model_step, model, ('hip_backward', 'sdpa'))

text = json.dumps(result, indent=1)
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text + '\n')
