"""The causal attention core: the library's HIP kernel (spq_causal_attention_fwd) against torch-ROCm's fused
scaled_dot_product_attention and the reference's explicit formula, in ONE process, the three alternated `--repeats` times,
HIP-event timing after warm-ups.

(a) the core alone at 8, 32 and 64 sequences x 12 or 16 heads x 1024 x 64, fp32: `SPAttention.core` under each setting (so SDPA
    and the explicit formula carry their head split / merge copies, as they do in the model), plus the kernel alone through
    the C ABI with its fraction of the 157.3 TFLOP/s fp32 matrix peak over the causal FLOP count 2 * 2 * B H d T (T + 1) / 2;
(b) one SPBlock eval forward at 32 x 1024 tokens, 4-bit min-max + LoRA r = 64, with the flag off (SDPA) and on.
Prints one JSON document; --out writes it to a file.  Only ratios within one run count (machines differ by several per cent)."""
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
ap.add_argument('--out', default=None)
args = ap.parse_args()
dev = torch.device('cuda:0')
PEAK_F32_MATRIX = 157.3e12
T, d, bits, r = 1024, 64, 4, 64
CORES = ('hip', 'sdpa', 'explicit')


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


def alternate(fn, set_core, cores):
    times = {c: [] for c in cores}
    for _ in range(args.repeats):
        for c in cores:
            set_core(c)
            times[c].append(time_ms(fn, args.iters))
    return {c: summary(times[c]) for c in cores}


result = {'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'iters': args.iters, 'unit': 'ms',
          'peak_f32_matrix_flops': PEAK_F32_MATRIX}
lib = pkg._lib.load()

# ---- (a) the core alone --------------------------------------------------------------------------------------------------------
for B, H in ((8, 12), (32, 12), (64, 12), (8, 16), (32, 16), (64, 16)):
    cfg = types.SimpleNamespace(n_embd=H * d, n_head=H, n_positions=T, layer_norm_epsilon=1e-5, bit_widths=[bits, 32],
                                lora_rank_per_bit={bits: r, 32: 0}, lora_alpha_per_bit={bits: 64, 32: 0},
                                quantizer_per_bit={bits: 'minmax', 32: None}, per_channel_quantization=True)
    att = pkg.SPAttention(cfg, [bits, 32]).to(dev).eval()
    qkv = torch.randn(B, T, 3 * H * d, generator=torch.Generator().manual_seed(B + H)).to(dev)
    with torch.no_grad():
        entry = alternate(lambda: att.core(qkv), lambda c: pkg.set_attention_core(att, c), CORES)
        pkg.set_attention_core(att, 'hip')
        y_hip = att.core(qkv)
        pkg.set_attention_core(att, 'explicit')
        entry['max_abs_diff_hip_vs_explicit'] = float((y_hip - att.core(qkv)).abs().max())
    out = torch.empty(B, T, H * d, device=dev)
    st = pkg._lib.stream_ptr(dev)
    kern = lambda: lib.spq_causal_attention_fwd(qkv.data_ptr(), B, T, H, d, out.data_ptr(), None, st)
    assert kern() == 0
    k = [time_ms(kern, args.iters) for _ in range(args.repeats)]
    flop = 2 * 2 * B * H * d * T * (T + 1) // 2
    entry['kernel'] = dict(summary(k), causal_flop=flop, fraction_of_f32_matrix_peak=flop / (statistics.median(k) * 1e-3) / PEAK_F32_MATRIX)
    entry['sdpa_over_hip'] = entry['sdpa']['median'] / entry['hip']['median']
    entry['explicit_over_hip'] = entry['explicit']['median'] / entry['hip']['median']
    result[f'core_{B}x{H}x{T}x{d}'] = entry
    del att, qkv, out, y_hip

# ---- (b) one SPBlock eval forward, 32 x 1024 tokens ---------------------------------------------------------------------------------
B, H, E = 32, 12, 768
cfg = types.SimpleNamespace(n_embd=E, n_head=H, n_positions=T, layer_norm_epsilon=1e-5, bit_widths=[bits, 32],
                            lora_rank_per_bit={bits: r, 32: 0}, lora_alpha_per_bit={bits: 64, 32: 0},
                            quantizer_per_bit={bits: 'minmax', 32: None}, per_channel_quantization=True)
torch.manual_seed(0)
blk = pkg.SPBlock(cfg, bit_widths=[bits, 32])
with torch.no_grad():
    for n, p in blk.named_parameters():
        if 'lora_B' in n: p.normal_(0, 0.01)
        elif p.dim() > 1 and 'lora_A' not in n: p.normal_(0, 0.02)
blk = blk.to(dev).eval()
gen = torch.Generator().manual_seed(7)
xs = [torch.randn(B, T, E, generator=gen).to(dev) for _ in range(2)]
pkg.calibrate_model(blk, bits, xs)
with torch.no_grad():
    entry = alternate(lambda: blk(xs[0]), lambda c: pkg.set_attention_core(blk, c), ('hip', 'sdpa'))
entry['sdpa_over_hip'] = entry['sdpa']['median'] / entry['hip']['median']
result['spblock_eval_32x1024_4bit'] = entry

text = json.dumps(result, indent=1)
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text + '\n')
