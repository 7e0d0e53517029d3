"""Times ops.softmax_uncertainty against the plain torch expression, the one that stores the (S, F, C, B) probabilities, on one
GPU: median of repeated runs after a warm-up, and the peak device memory of each above the inputs.  Not collected by pytest.
    python tests/native/uncertainty_time.py [S F C B]          (default 3 10 10 100000)"""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from vargp_amd import ops  # noqa: E402


def composed(mu, var, eps):
    logp = torch.log_softmax(mu.unsqueeze(1) + var.sqrt().unsqueeze(1) * eps, dim=2)
    p = logp.exp()
    probs = p.mean((0, 1))
    total = -torch.xlogy(probs, probs).sum(0)
    expected = (-(p * logp).sum(2)).mean((0, 1))
    return probs.t().contiguous(), total, expected, (total - expected).clamp_min(0)


def measure(fn, args, warmup=5, reps=30):
    for _ in range(warmup):
        fn(*args)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn(*args)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
        del out
    return sorted(times)[len(times) // 2], (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    S, F, C, B = (int(v) for v in sys.argv[1:5]) if len(sys.argv) >= 5 else (3, 10, 10, 100000)
    gen = torch.Generator(device='cuda').manual_seed(0)
    mu = torch.randn(S, C, B, device='cuda', generator=gen)
    var = 0.01 + 0.5 * torch.rand(S, C, B, device='cuda', generator=gen)
    eps = torch.randn(S, F, C, B, device='cuda', generator=gen)
    fused_ms, fused_mb = measure(ops.softmax_uncertainty, (mu, var, eps))
    torch_ms, torch_mb = measure(composed, (mu, var, eps))
    got, want = ops.softmax_uncertainty(mu, var, eps), composed(mu, var, eps)
    err = max(((a - b).norm() / b.norm()).item() for a, b in zip(got, want))
    print(f'S{S} F{F} C{C} B{B}: fused {fused_ms:.3f} ms, peak +{fused_mb:.1f} MiB (scratch pool included once grown: '
          f'{ops.scratch(0, "cuda").numel() * 4 / 2 ** 20:.1f} MiB); torch {torch_ms:.3f} ms, peak +{torch_mb:.1f} MiB; '
          f'worst rel_l2 between the two {err:.1e}')


if __name__ == '__main__':
    main()
