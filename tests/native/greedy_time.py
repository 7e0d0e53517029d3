"""init.greedy_inducing (ops.greedy_select, csrc/greedy.hip) at the Split-MNIST shape (N, D, C, M) = (12000, 784, 10, 100) with the
default 4096 candidates, from an empty start (k0 = 0) and from 400 earlier inducing points (k0 = 400), against two comparisons on
the same GPU: init.kmeans_inducing at its default 20 iterations, and the same M steps composed from torch ops (a kernel column, a
matrix-vector downdate and a host-visible argmax per step and set: the baseline -- the library had no counterpart before).  The
step kernel alone is timed too (ops.greedy_select on prepared candidates, prefill excluded) and its traffic estimate
sum_k Nc (D + k0 + k) 4 bytes per set over that time is reported as bytes/s.  Timed alternately with device events (median and
minimum of REPS calls after a warm-up).  Feeds the greedy section of DESIGN.md.  GPU box only."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from vargp_amd import init, ops  # noqa: E402

dev = torch.device('cuda', 0)
WARM, REPS = 2, 7
N, D, C, M, NC = 12000, 784, 10, 100, 4096
g = torch.Generator(device=dev).manual_seed(0)
x = torch.rand(N, D, device=dev, generator=g) * (torch.rand(N, D, device=dev, generator=g) < 0.19)      # MNIST-like pixels
torch.manual_seed(0)
theta = torch.cat([torch.full((D,), math.log(init.median_lengthscale(x))), torch.tensor([math.log(0.5)])]).to(dev)
z_prev = torch.stack([x[torch.randperm(N, device=dev, generator=g)[:400]] for _ in range(C)])
cand = init.draw_candidates(N, C, NC).to(dev, torch.int32)


def torch_steps(LT0, d0):
    """the M steps of one call composed from torch ops, all sets batched; -> pick (C, M)"""
    ls, g2 = theta[:-1].exp(), (2.0 * theta[-1]).exp()
    xc = x[cand.long()] / ls                                             # (C, Nc, D): gathered once, outside the steps' traffic
    k0 = 0 if LT0 is None else LT0.shape[1]
    LT = torch.zeros(C, k0 + M, NC, device=dev)
    if k0:
        LT[:, :k0] = LT0
    d = d0.clone() if k0 else g2.expand(C, NC).clone()
    sel = torch.zeros(C, NC, dtype=torch.bool, device=dev)
    pick = torch.zeros(C, M, dtype=torch.int64, device=dev)
    ar = torch.arange(C, device=dev)
    for k in range(M):
        key = torch.where(sel, -1.0, torch.where(d > ops.JITTER, d, 0.0))
        p = key.argmax(-1)
        pick[:, k] = p
        p_host = p.tolist()                                              # the host-visible argmax of a step-by-step composition
        dp = d[ar, p]
        col = g2 * (-0.5 * (xc - xc[ar, p].unsqueeze(1)).square().sum(-1)).exp()
        c = col - torch.einsum('cjn,cj->cn', LT[:, :k0 + k], LT[:, :k0 + k][ar, :, p])
        row = c / dp.sqrt().unsqueeze(-1)
        LT[:, k0 + k] = row
        d = (d - row * row).clamp_min(0.0)
        sel[ar, p] = True
        del p_host
    return pick


def timed(fn):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    out = fn()
    e[1].record()
    e[1].synchronize()
    return e[0].elapsed_time(e[1]), out


for k0 in (0, 400):
    zp = z_prev if k0 else None
    LT0 = d0 = None
    if k0:
        pre = [init.whitened_cross(theta, z_prev[c], x[cand[c].long()]) for c in range(C)]
        LT0, d0 = torch.stack([p[0] for p in pre]), torch.stack([p[1] for p in pre])
    fns = {
        'greedy_inducing': lambda: init.greedy_inducing(x, C, M, theta, z_prev=zp, cand=cand.cpu().long()),
        'greedy_select': lambda: ops.greedy_select(theta, x, cand, LT0, d0, M=M)[0],
        'torch_steps': lambda: torch_steps(LT0, d0),
        'kmeans_inducing': lambda: init.kmeans_inducing(x, C, M),
    }
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    outs = {}
    for _ in range(REPS):
        for name, fn in fns.items():
            ms, outs[name] = timed(fn)
            t[name].append(ms)
    nbytes = C * sum(NC * (D + k0 + k) * 4 for k in range(M))
    res = dict(N=N, D=D, C=C, M=M, Nc=NC, k0=k0, reps=REPS, step_bytes_estimate=nbytes,
               picks_differing_from_torch=int((outs['greedy_select'].long() != outs['torch_steps']).sum()))
    for name, v in t.items():
        res[f'{name}_ms_median'], res[f'{name}_ms_min'] = statistics.median(v), min(v)
    res['greedy_select_TBps_median'] = nbytes / (res['greedy_select_ms_median'] * 1e-3) / 1e12
    res['speedup_over_torch_median'] = res['torch_steps_ms_median'] / res['greedy_select_ms_median']
    print(json.dumps(res), flush=True)
