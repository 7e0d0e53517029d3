"""One iteration of fit_q_softmax_'s data work -- the marginals pass, the softmax site pass and the moments pass -- at N = 60000
points, D = 784, C = 10 classes, F = 32 draws per point, RBF, Mt = 100 and 200: the fused route (ops.site_marginals) against the
composed route (sites.composed_softmax_marginals: the gram op and ops.bgemm on tiles of 8192 points); ops.softmax_sites and
ops.gram_moments_v are the same on both.  Every pass is timed on its own, alternately, with device events (median and minimum of
REPS calls after a warm-up).  Also reports the largest difference of the two routes' marginals relative to the largest entry.
Feeds the softmax section of DESIGN.md.  GPU box only."""
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
C, D, N, F = 10, 784, 60000, 32


def timed(fn):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    out = fn()
    e[1].record()
    e[1].synchronize()
    return e[0].elapsed_time(e[1]), out


for Mt in (100, 200):
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(N, D, device=dev, generator=g)
    Z = torch.stack([X[torch.randperm(N, device=dev, generator=g)[:Mt]] for _ in range(C)]).contiguous()
    y = torch.randint(0, C, (N,), device=dev, generator=g)
    theta = torch.cat([torch.full((D,), math.log(0.8 * math.sqrt(D))), torch.tensor([0.0])]).to(dev)
    alpha = 0.3 * torch.randn(C, Mt, device=dev, generator=g) / math.sqrt(Mt)
    R = torch.randn(C, Mt, Mt, device=dev, generator=g)
    Q = (0.5 / Mt ** 2) * ops.bgemm(R, R.mT)
    Q = (0.5 * (Q + Q.mT)).contiguous()
    mu, var = ops.site_marginals(theta, Z, X, alpha, Q, 0)
    lam1, lam2, _ = ops.softmax_sites(mu, var, y, None, F, seed=1)

    fns = {'marginals_fused': lambda: ops.site_marginals(theta, Z, X, alpha, Q, 0),
           'marginals_composed': lambda: sites.composed_softmax_marginals(theta, Z, X, alpha, Q, 0),
           'softmax_sites': lambda: ops.softmax_sites(mu, var, y, None, F, seed=1),
           'gram_moments_v': lambda: ops.gram_moments_v(theta, Z, X, lam2, lam1, 0)}
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t, outs = {name: [] for name in fns}, {}
    for _ in range(REPS):
        for name, fn in fns.items():
            ms, outs[name] = timed(fn)
            t[name].append(ms)
    a, b = outs['marginals_fused'], outs['marginals_composed']
    res = dict(N=N, D=D, Mt=Mt, C=C, F=F, reps=REPS, chunks=ops.site_moments_chunks(C, Mt, N, D),
               mu_max_rel_diff=((a[0] - b[0]).abs().max() / b[0].abs().max()).item(),
               var_max_rel_diff=((a[1] - b[1]).abs().max() / b[1].abs().max()).item())
    for name, v in t.items():
        res[f'{name}_ms_median'], res[f'{name}_ms_min'] = statistics.median(v), min(v)
    rest = res['softmax_sites_ms_median'] + res['gram_moments_v_ms_median']
    res['iteration_fused_ms'] = res['marginals_fused_ms_median'] + rest
    res['iteration_composed_ms'] = res['marginals_composed_ms_median'] + rest
    res['marginals_composed_over_fused'] = res['marginals_composed_ms_median'] / res['marginals_fused_ms_median']
    print(json.dumps(res), flush=True)
    del X, Z
