"""One value + gradient of the softmax site bound -- an M-step's unit of work in fit_softmax_sites_ -- at C = 10 classes, Mt = 100,
D = 784, N = 60000, n_f = 32, RBF: the fused route (ops.softmax_site_bound_diff: ops.site_marginals, ops.softmax_sites |
ops.softmax_site_grads, ops.site_transport_bwd, ops.gram_moments) against the composed route (sites.composed_softmax_site_bound:
the gram op, ops.matmul and fp32 elementwise torch on tiles of 8192 points and an explicit noise tensor, which it is handed
ready-made here).  Timed alternately with device events (median and minimum of REPS calls after a warm-up), on a device that a
first untimed pass has brought to its clocks.  Also reports the largest difference of the two gZ relative to the largest entry.
Feeds the softmax site bound section of DESIGN.md.  GPU box only."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from vargp_amd import ops, sites  # noqa: E402

dev = torch.device('cuda', 0)
WARM, REPS = 2, 5
C, Mt, D, N, F, SEED = 10, 100, 784, 60000, 32, 0


def timed(fn):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    out = fn()
    e[1].record()
    e[1].synchronize()
    return e[0].elapsed_time(e[1]), out


g = torch.Generator(device=dev).manual_seed(0)
X = torch.randn(N, D, device=dev, generator=g)
Z = torch.stack([X[torch.randperm(N, device=dev, generator=g)[:Mt]] for _ in range(C)]).contiguous()
y = torch.randint(0, C, (N,), device=dev, generator=g)
theta = torch.cat([torch.full((D,), math.log(0.8 * math.sqrt(D))), torch.tensor([0.0])]).to(dev)
alpha = 0.3 * torch.randn(C, Mt, device=dev, generator=g) / math.sqrt(Mt)
R = torch.randn(C, Mt, Mt, device=dev, generator=g)
Q = (0.5 / Mt ** 2) * ops.bgemm(R, R.mT)
Q = (0.5 * (Q + Q.mT)).contiguous()
eps = ops.softmax_site_noise(SEED, F, C, N, device=dev)


def value_and_grad(bound, **kw):
    leaves = [t.clone().requires_grad_(True) for t in (theta, Z, alpha, Q)]
    val = bound(leaves[0], leaves[1], X, leaves[2], leaves[3], y, None, F, SEED, **kw)
    return val.detach(), torch.autograd.grad(val.sum(), leaves)


fns = {'fused': lambda: value_and_grad(ops.softmax_site_bound_diff),
       'composed': lambda: value_and_grad(sites.composed_softmax_site_bound, eps=eps)}
for _ in range(WARM):
    for fn in fns.values():
        fn()
torch.cuda.synchronize()
t, outs = {name: [] for name in fns}, {}
for _ in range(REPS):
    for name, fn in fns.items():
        ms, outs[name] = timed(fn)
        t[name].append(ms)
gz = [outs[name][1][1] for name in ('fused', 'composed')]
res = dict(N=N, D=D, Mt=Mt, C=C, n_f=F, reps=REPS, chunks=ops.site_transport_bwd_chunks(C, Mt, N, D),
           value_fused=outs['fused'][0].item(), value_composed=outs['composed'][0].item(),
           gZ_max_rel_diff=((gz[0] - gz[1]).abs().max() / gz[1].abs().max()).item())
for name, v in t.items():
    res[f'{name}_ms_median'], res[f'{name}_ms_min'] = statistics.median(v), min(v)
res['composed_over_fused_median'] = res['composed_ms_median'] / res['fused_ms_median']
print(json.dumps(res), flush=True)
