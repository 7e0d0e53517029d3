"""One forward + backward of ops.site_bound_diff (ops.site_moments; then ops.site_bound_bwd and one ops.gram_moments call) against
the same gradient assembled from the entries the library had before vargp_site_bound_bwd, at C = 10 outputs, Mt = 200, N = 1e5,
D = 784 and D = 8, Bernoulli-probit, RBF.  The assembled route has three legs:
  1. the per-point terms by the structure of the site pass: ops.site_moments' lam2 gives gv = -lam2 / 2 (log-concave likelihood:
     nothing is clamped), and gm = w dmu comes as sites.composed_site_moments forms it -- the gram op, ops.bgemm and
     ops.lik_nll_bwd on tiles of 8192 points (K of a tile is stored);
  2. two ops.gram_moments calls give galpha (c with y = gm, w = 1) and gQ (-Phi with w = gv);
  3. two ops.gram_moments_bwd calls give gK's share of gZ and gtheta: (gPhi = Q / 2, w = -2 gv) and (gc = alpha, w = 1, y = gm).
Timed alternately with device events (median and minimum of REPS calls after a warm-up), on a device that a first untimed pass has
brought to its clocks.  Also reports the largest difference of the two gZ relative to the largest entry.  Feeds the site-bound
section of DESIGN.md.  GPU box only."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from vargp_amd import ops  # noqa: E402

dev = torch.device('cuda', 0)
WARM, REPS = 2, 5
C, Mt, N = 10, 200, 100_000
TILE = 8192


def timed(fn):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    out = fn()
    e[1].record()
    e[1].synchronize()
    return e[0].elapsed_time(e[1]), out


for D in (784, 8):
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(N, D, device=dev, generator=g)
    Z = torch.stack([X[torch.randperm(N, device=dev, generator=g)[:Mt]] for _ in range(C)]).contiguous()
    y = (torch.rand(C, N, device=dev, generator=g) < 0.5).float()
    theta = torch.cat([torch.full((D,), math.log(0.8 * math.sqrt(D))), torch.tensor([0.0])]).to(dev)
    alpha = 0.3 * torch.randn(C, Mt, device=dev, generator=g) / math.sqrt(Mt)
    R = torch.randn(C, Mt, Mt, device=dev, generator=g)
    Q = (0.5 / Mt ** 2) * ops.bgemm(R, R.mT)
    Q = (0.5 * (Q + Q.mT)).contiguous()
    seed = torch.ones(C, device=dev)

    def fused():
        leaves = [t.clone().requires_grad_(True) for t in (theta, Z, alpha, Q)]
        val = ops.site_bound_diff(leaves[0], leaves[1], X, leaves[2], leaves[3], y, None, 'bernoulli', (0,), 0)
        return torch.autograd.grad(val.sum(), leaves)

    def assembled():
        lam2, c, sums = ops.site_moments(theta, Z, X, alpha, Q, y, None, 'bernoulli', (0,), 0)
        gv = -0.5 * lam2
        gm = torch.empty_like(lam2)
        th = theta.view(1, -1)
        for n0 in range(0, N, TILE):
            K = ops.rbf_gram(th, Z, X[n0:n0 + TILE].contiguous(), True)[0]
            mu = ops.bgemm(alpha.unsqueeze(-2), K).squeeze(-2)
            seedv = torch.ones((), device=dev)
            var = (1.0 - (K * ops.bgemm(Q, K)).sum(-2)).clamp_min(0.0).contiguous()
            gmu, gvar = torch.empty_like(mu), torch.empty_like(var)
            yt = y[:, n0:n0 + TILE].contiguous()
            ops.lik_nll_bwd('bernoulli', mu.contiguous().unsqueeze(0), var.unsqueeze(0), ops.lik_target('bernoulli', yt, C, yt.size(1)),
                            (0,), seedv, gmu.unsqueeze(0), gvar.unsqueeze(0), None)
            gm[:, n0:n0 + TILE] = -gmu
        ones = torch.ones_like(gm)
        Phi = ops.gram_moments(theta, Z, X, gv, gv, 0)[0]
        galpha = ops.gram_moments(theta, Z, X, None, gm, 0)[1]
        gZ1, gth1 = ops.gram_moments_bwd(theta, Z, X, (-2.0 * gv).contiguous(), gm, (0.5 * Q).contiguous(), torch.zeros_like(alpha), 0)
        gZ2, gth2 = ops.gram_moments_bwd(theta, Z, X, ones, gm, torch.zeros_like(Q), alpha, 0)
        return gth1 + gth2, gZ1 + gZ2, galpha, -Phi

    fns = {'fused': fused, 'assembled': assembled}
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t, outs = {name: [] for name in fns}, {}
    for _ in range(REPS):
        for name, fn in fns.items():
            ms, outs[name] = timed(fn)
            t[name].append(ms)
    res = dict(N=N, D=D, Mt=Mt, C=C, reps=REPS, chunks=ops.site_bound_bwd_chunks(C, Mt, N, D),
               gZ_max_rel_diff=((outs['fused'][1] - outs['assembled'][1]).abs().max() / outs['assembled'][1].abs().max()).item(),
               gQ_max_rel_diff=((outs['fused'][3] - outs['assembled'][3]).abs().max() / outs['assembled'][3].abs().max()).item())
    for name, v in t.items():
        res[f'{name}_ms_median'], res[f'{name}_ms_min'] = statistics.median(v), min(v)
    res['assembled_over_fused_median'] = res['assembled_ms_median'] / res['fused_ms_median']
    print(json.dumps(res), flush=True)
    del X, Z, y
