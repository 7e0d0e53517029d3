"""One Lloyd iteration on the fused kernels (ops.kmeans_assign + ops.kmeans_update, csrc/kmeans.hip) against the torch composition
it replaces -- cdist, argmin, index_add_ and a divide per set -- at the Split-MNIST task (N, G, K, D) = (12000, 2, 100, 784) and at
Permuted-MNIST (60000, 10, 100, 784).  The two are timed alternately with device events (median and minimum of REPS calls after
a warm-up), assign and update split by the same events, and each side's peak memory above the inputs is read from
torch.cuda.max_memory_allocated.  Feeds the k-means section of DESIGN.md.  GPU box only."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from vargp_amd import ops  # noqa: E402

dev = torch.device('cuda', 0)
WARM, REPS = 3, 15
g = torch.Generator(device=dev).manual_seed(0)


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


for N, G, K, D in ((12000, 2, 100, 784), (60000, 10, 100, 784)):
    x = torch.rand(N, D, device=dev, generator=g) * (torch.rand(N, D, device=dev, generator=g) < 0.19)      # MNIST-like pixels
    z = torch.stack([x[torch.randperm(N, device=dev, generator=g)[:K]] for _ in range(G)])

    def fused():
        e = events(3)
        e[0].record()
        label, d2 = ops.kmeans_assign(x, z)
        e[1].record()
        z_new, count = ops.kmeans_update(x, label, z)
        e[2].record()
        return e, (label, z_new)

    def composed():
        e = events(3)
        e[0].record()
        label = torch.stack([torch.cdist(x, z[s]).argmin(-1) for s in range(G)])
        e[1].record()
        z_new = torch.empty_like(z)
        for s in range(G):
            sums = torch.zeros(K, D, device=dev).index_add_(0, label[s], x)
            cnt = torch.bincount(label[s], minlength=K).unsqueeze(-1)
            z_new[s] = torch.where(cnt > 0, sums / cnt.clamp_min(1), z[s])
        e[2].record()
        return e, (label, z_new)

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        out = fn()
        torch.cuda.synchronize()
        del out
        return torch.cuda.max_memory_allocated(dev) - base

    for _ in range(WARM):
        fused(), composed()
    torch.cuda.synchronize()
    t = {'fused': ([], []), 'composed': ([], [])}
    for _ in range(REPS):
        for name, fn in (('fused', fused), ('composed', composed)):
            e, out = fn()
            e[2].synchronize()
            t[name][0].append(e[0].elapsed_time(e[1]))
            t[name][1].append(e[1].elapsed_time(e[2]))
            if name == 'fused':
                a = out
            else:
                b = out
    res = dict(N=N, G=G, K=K, D=D, reps=REPS, assign_gflop=2.0 * N * G * K * D / 1e9,
               labels_differing=int((a[0].long() != b[0]).sum()), centres_max_abs_diff=(a[1] - b[1]).abs().max().item(),
               fused_peak_bytes=peak(fused), composed_peak_bytes=peak(composed))
    for name in t:
        asg, upd = t[name]
        tot = [p + q for p, q in zip(asg, upd)]
        res.update({f'{name}_ms_median': statistics.median(tot), f'{name}_ms_min': min(tot),
                    f'{name}_assign_ms_median': statistics.median(asg), f'{name}_update_ms_median': statistics.median(upd)})
    res['speedup_median'] = res['composed_ms_median'] / res['fused_ms_median']
    print(json.dumps(res), flush=True)
    del x, z, a, b
