"""The language-model loss alone, forward + backward: ``lm_cross_entropy`` (csrc/spq_lm_loss.hip) against the reference's two torch
lines (shift, F.cross_entropy), in ONE process, the two alternated `--repeats` times, HIP-event timing around `--iters` steps, at
8 x 1024 x 50257 and 2 x 1024 x 50257 fp32 logits.  Reports median (min - max) and torch.cuda.max_memory_allocated of each
variant, the library's launches alone through the C ABI (no autograd, no allocation), and the bytes per logit element each time
implies at the HBM copy ceiling.  Prints one JSON document; --out writes it (default profiles/lm_loss_bench.json)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import llm_qat_on_gpt2_amd as pkg  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--repeats', type=int, default=5)
ap.add_argument('--iters', type=int, default=10)
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lm_loss_bench.json'))
args = ap.parse_args()
dev = torch.device('cuda:0')
HBM_COPY_CEILING = 6.3e12            # bytes / s, read + write, what a streaming copy reaches on this part
T, V = 1024, 50257


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


def summary(v, elements):
    med = statistics.median(v)
    return {'median': med, 'min': min(v), 'max': max(v), 'runs': v,
            'bytes_per_element_at_copy_ceiling': med * 1e-3 * HBM_COPY_CEILING / elements}


def torch_loss(logits, labels):
    shift_logits = logits[..., :-1, :].contiguous()
    shift_labels = labels[..., 1:].contiguous()
    return F.cross_entropy(shift_logits.view(-1, shift_logits.size(-1)), shift_labels.view(-1))


result = {'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'iters': args.iters, 'unit': 'ms',
          'hbm_copy_ceiling_bytes_per_s': HBM_COPY_CEILING}
lib = pkg._lib.load()
for B in (8, 2):
    gen = torch.Generator().manual_seed(B)
    logits = (torch.randn(B, T, V, generator=gen) * 3.0).to(dev).requires_grad_(True)
    labels = torch.randint(V, (B, T), generator=gen).to(dev)
    elements = B * T * V
    base = torch.cuda.memory_allocated()
    variants = {'hip': pkg.lm_cross_entropy, 'torch': torch_loss}
    times, mem, value = {v: [] for v in variants}, {}, {}
    for _ in range(args.repeats):
        for name, loss_fn in variants.items():
            def step():
                logits.grad = None
                loss = loss_fn(logits, labels)
                loss.backward()
                return loss
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            times[name].append(time_ms(step, args.iters))
            mem[name] = torch.cuda.max_memory_allocated()
            value[name] = float(step())
    entry = {name: dict(summary(times[name], elements), peak_bytes=mem[name], peak_bytes_above_the_logits=mem[name] - base,
                        loss=value[name]) for name in variants}
    entry['logits_bytes'] = elements * 4
    entry['torch_over_hip'] = entry['torch']['median'] / entry['hip']['median']
    # the library's launches alone, through the C ABI
    x = logits.detach()
    nll, lse = torch.empty(B, T, device=dev), torch.empty(2, B, T, device=dev)
    loss, count = torch.empty(2, device=dev), torch.empty(1, dtype=torch.int64, device=dev)
    one = torch.ones(1, device=dev)
    dlogits = torch.empty_like(x)
    st = pkg._lib.stream_ptr(dev)
    fwd = lambda: lib.spq_lm_cross_entropy_fwd(x.data_ptr(), labels.data_ptr(), B, T, V, 1, -100, nll.data_ptr(), lse.data_ptr(),
                                               loss.data_ptr(), count.data_ptr(), st)
    bwd = lambda: lib.spq_lm_cross_entropy_bwd(x.data_ptr(), labels.data_ptr(), lse.data_ptr(), B, T, V, 1, -100, one.data_ptr(), None,
                                               count.data_ptr(), dlogits.data_ptr(), st)
    assert fwd() == 0 and bwd() == 0
    entry['kernel_forward'] = summary([time_ms(fwd, 20) for _ in range(args.repeats)], elements)      # reads 4 B per element
    entry['kernel_backward'] = summary([time_ms(bwd, 20) for _ in range(args.repeats)], elements)     # reads 4, writes 4
    result[f'loss_{B}x{T}x{V}'] = entry
    del logits, labels, x, dlogits

text = json.dumps(result, indent=1)
print(text)
if args.out:
    with open(args.out, 'w') as f:
        f.write(text + '\n')
