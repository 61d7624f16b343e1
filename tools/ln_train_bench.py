"""SwitchableLayerNorm under autograd: the HIP forward / backward pair (fuse_backward = True) against the composed formula on
stock torch ops (fuse_backward = False, the behaviour before the pair existed), in ONE process, the two alternated `--repeats`
times, HIP-event timing.

(a) the module alone, forward + backward, at 8192 x 768 and 32768 x 768 -- plus the library's kernels alone against their
    algorithmic bytes (forward 8 B / element, backward 12 B / element) as a fraction of the 6.3 TB/s copy ceiling;
(b) one SPBlock and the 12-layer SPModel, training step (forward + backward), 8 x 1024 tokens, 4-bit min-max + LoRA r = 64, base
    weights frozen, with torch.cuda.max_memory_allocated.
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
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--layers', type=int, default=12)
ap.add_argument('--out', default=None)
args = ap.parse_args()
dev = torch.device('cuda:0')
COPY_CEILING = 6.3e12
E, bits, r = 768, 4, 64


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


def alternate(fn_of_mode, setup_mode):
    """{mode: summary}: fused / composed alternated args.repeats times, peak memory of the last repeat"""
    times, mem = {'fused': [], 'composed': []}, {}
    for _ in range(args.repeats):
        for mode in ('fused', 'composed'):
            setup_mode(mode == 'fused')
            torch.cuda.reset_peak_memory_stats()
            times[mode].append(time_ms(fn_of_mode, args.iters))
            mem[mode] = torch.cuda.max_memory_allocated()
    return {m: dict(summary(times[m]), peak_bytes=mem[m]) for m in times}


result = {'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'iters': args.iters, 'unit': 'ms'}

# ---- (a) the module alone ---------------------------------------------------------------------------------------------------------
lib = pkg._lib.load()
for rows in (8192, 32768):
    ln = pkg.SwitchableLayerNorm(E, precision_levels=[bits, 32]).to(dev)
    ln.set_precision(bits)
    gen = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, E, generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(rows, E, generator=gen).to(dev)

    def step():
        x.grad = None
        ln.zero_grad(set_to_none=True)
        ln(x).backward(g)
    entry = alternate(step, lambda fused: setattr(ln, 'fuse_backward', fused))
    # the kernels alone, through the C ABI (no autograd, no allocation)
    w, b = ln.weights[str(bits)].detach(), ln.biases[str(bits)].detach()
    xd = x.detach()
    out, dx, mean, den = torch.empty_like(xd), torch.empty_like(xd), torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    dw, db = torch.empty_like(w), torch.empty_like(w)
    ws = torch.empty(lib.spq_layernorm_bwd_workspace_bytes(rows, E), dtype=torch.uint8, device=dev)
    st = pkg._lib.stream_ptr(dev)
    fwd = lambda: lib.spq_layernorm_fwd_stats(xd.data_ptr(), rows, E, w.data_ptr(), b.data_ptr(), 1e-5, out.data_ptr(),
                                              mean.data_ptr(), den.data_ptr(), st)
    bwd = lambda: lib.spq_layernorm_bwd(g.data_ptr(), xd.data_ptr(), mean.data_ptr(), den.data_ptr(), w.data_ptr(), rows, E,
                                        dx.data_ptr(), dw.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), st)
    assert fwd() == 0 and bwd() == 0
    kf = [time_ms(fwd, 50) for _ in range(args.repeats)]
    kb = [time_ms(bwd, 50) for _ in range(args.repeats)]
    n = rows * E
    entry['kernel_forward'] = dict(summary(kf), bytes=8 * n, fraction_of_copy_ceiling=8 * n / (statistics.median(kf) * 1e-3) / COPY_CEILING)
    entry['kernel_backward'] = dict(summary(kb), bytes=12 * n, fraction_of_copy_ceiling=12 * n / (statistics.median(kb) * 1e-3) / COPY_CEILING)
    result[f'module_{rows}x{E}'] = entry
    del x, g, out, dx

# ---- (b) one SPBlock and the SPModel, training step ---------------------------------------------------------------------------------
B, T = 8, 1024
cfg = types.SimpleNamespace(vocab_size=1024, n_positions=T, n_embd=E, n_layer=args.layers, n_head=12, layer_norm_epsilon=1e-5,
                            bit_widths=[bits, 32], lora_rank_per_bit={bits: r, 32: 0}, lora_alpha_per_bit={bits: 64, 32: 0},
                            quantizer_per_bit={bits: 'minmax', 32: None}, per_channel_quantization=True)


def prepare(model, batches, forward=None):
    torch.manual_seed(0)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if 'lora_B' in n: p.normal_(0, 0.01)
            elif p.dim() > 1 and 'lora_A' not in n: p.normal_(0, 0.02)
    model = model.to(dev).eval()
    pkg.calibrate_model(model, bits, batches, forward=forward)
    model.train()
    for m in model.modules():
        if m.__class__.__name__ == 'SPLinearWithLoRA':                # base weights frozen (main_sp.py:83)
            for p in m.linear.parameters():
                p.requires_grad_(False)
    return model


def set_ln(model):
    def f(fused):
        for m in model.modules():
            if isinstance(m, pkg.SwitchableLayerNorm):
                m.fuse_backward = fused
    return f


gen = torch.Generator().manual_seed(7)
xb = torch.randn(B, T, E, generator=gen).to(dev)
gb = torch.randn(B, T, E, generator=gen).to(dev)
blk = prepare(pkg.SPBlock(cfg, bit_widths=[bits, 32]), [xb, torch.randn(B, T, E, generator=gen).to(dev)])
xg = xb.clone().requires_grad_(True)


def block_step():
    xg.grad = None
    blk.zero_grad(set_to_none=True)
    blk(xg).backward(gb)
result['spblock_8x1024'] = alternate(block_step, set_ln(blk))
del blk

ids = torch.randint(0, cfg.vocab_size, (B, T), generator=gen).to(dev)
model = prepare(pkg.SPModel(cfg), [ids, torch.randint(0, cfg.vocab_size, (B, T), generator=gen).to(dev)])


def model_step():
    model.zero_grad(set_to_none=True)
    model(ids).backward(gb)
result[f'spmodel_{args.layers}layer_8x1024'] = alternate(model_step, set_ln(model))

for k, v in result.items():
    if isinstance(v, dict) and 'fused' in v:
        v['composed_over_fused'] = v['composed']['median'] / v['fused']['median']
text = json.dumps(result, indent=1)
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text + '\n')
