"""One iteration of fit_q_newton_'s data work -- the site pass and the moments pass -- at N = 1e5 and 1e6 points, Mt = 100 and 200,
D = 784, C = 10 outputs, Bernoulli-probit, RBF: the fused route (ops.site_moments + ops.gram_moments) against the composed route
(sites.composed_site_moments: the gram op, ops.bgemm and ops.lik_nll_bwd on tiles of 8192 points, + the same ops.gram_moments),
which is built from the per-op kernels the library had before csrc/sites.hip.  Timed alternately with device events (median and
minimum of REPS calls after a warm-up), on a device that a first untimed pass has brought to its clocks.  Also reports the largest
difference of the two c relative to the largest entry.  Feeds the sites section of DESIGN.md.  GPU box only."""
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
C, D = 10, 784


def timed(fn):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    out = fn()
    e[1].record()
    e[1].synchronize()
    return e[0].elapsed_time(e[1]), out


for N in (100_000, 1_000_000):
    for Mt in (100, 200):
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn(N, D, device=dev, generator=g)
        Z = torch.stack([X[torch.randperm(N, device=dev, generator=g)[:Mt]] for _ in range(C)]).contiguous()
        y = (torch.rand(C, N, device=dev, generator=g) < 0.5).float()
        theta = torch.cat([torch.full((D,), math.log(0.8 * math.sqrt(D))), torch.tensor([0.0])]).to(dev)
        alpha = 0.3 * torch.randn(C, Mt, device=dev, generator=g) / math.sqrt(Mt)
        R = torch.randn(C, Mt, Mt, device=dev, generator=g)
        Q = (0.5 / Mt ** 2) * ops.bgemm(R, R.mT)
        Q = (0.5 * (Q + Q.mT)).contiguous()

        def iteration(site_pass):
            lam2, c, sums = site_pass(theta, Z, X, alpha, Q, y, None, 'bernoulli', (0,), 0)
            return c, ops.gram_moments(theta, Z, X, lam2, lam2, 0)[0]

        fns = {'fused': lambda: iteration(ops.site_moments), 'composed': lambda: iteration(sites.composed_site_moments)}
        for _ in range(WARM):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t, outs = {name: [] for name in fns}, {}
        for _ in range(REPS):
            for name, fn in fns.items():
                ms, outs[name] = timed(fn)
                t[name].append(ms)
        res = dict(N=N, D=D, Mt=Mt, C=C, reps=REPS, chunks=ops.site_moments_chunks(C, Mt, N, D),
                   c_max_rel_diff=((outs['fused'][0] - outs['composed'][0]).abs().max() / outs['composed'][0].abs().max()).item())
        for name, v in t.items():
            res[f'{name}_ms_median'], res[f'{name}_ms_min'] = statistics.median(v), min(v)
        res['composed_over_fused_median'] = res['composed_ms_median'] / res['fused_ms_median']
        print(json.dumps(res), flush=True)
        del X, Z, y
