"""VARGP.loo at N = 60000 points, Mt = 100 inducing points, D = 784, C = 10 outputs, RBF, for a Bernoulli-probit and a softmax model
after two iterations of their site fits: the fused route (ops.site_cavity, or ops.site_marginals_s + ops.softmax_sites for the
softmax) against the composed route (loo.composed_site_cavity / composed_marginals_s: the gram op and ops.matmul on tiles of 8192
points), and -- the whole call, and the kernel ops.site_cavity alone -- against ops.site_moments ALONE at the same shape and q: the expectation being one site pass plus one (Mv x Mt x 64)
MFMA product per tile of 64 columns, well under 2 x.  Timed alternately with device events (median and minimum of REPS calls after
a warm-up) on a device that a first untimed pass has brought to its clocks; reports the shader clock the runtime names.  Also
reports the largest difference of the two routes' cavity moments relative to the largest entry, over the points both call stable.
Feeds the loo section of DESIGN.md.  GPU box only."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from vargp_amd import ops, sites  # noqa: E402
from vargp_amd.kernels import RBFKernel  # noqa: E402
from vargp_amd.likelihoods import BernoulliLikelihood, MulticlassSoftmax  # noqa: E402
from vargp_amd.vargp import VARGP  # noqa: E402
from vargp_amd.whitened import Frame, alpha_Q, read_q  # noqa: E402

dev = torch.device('cuda', 0)
WARM, REPS = 2, 5
N, M, D, C = 60_000, 100, 784, 10


def timed(fn):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    out = fn()
    e[1].record()
    e[1].synchronize()
    return e[0].elapsed_time(e[1]), out


def clock_mhz():
    try:
        return torch.cuda.clock_rate(dev)
    except Exception:                                                 # (no management library next to this torch build)
        return None


g = torch.Generator(device=dev).manual_seed(0)
X = torch.randn(N, D, device=dev, generator=g)
labels = torch.randint(0, C, (N,), device=dev, generator=g)
z = torch.stack([X[torch.randperm(N, device=dev, generator=g)[:M]] for _ in range(C)]).cpu()

for name in ('probit', 'softmax'):
    torch.manual_seed(0)
    kern = RBFKernel(D, map_est=True)
    with torch.no_grad():
        kern.log_mean[:D] = math.log(0.8 * math.sqrt(D))
    lik = BernoulliLikelihood(link='probit') if name == 'probit' else MulticlassSoftmax(n_f=10)
    gp = VARGP(z, kern, lik, n_var_samples=1).to(dev)
    fit = (gp.fit_q_newton_ if name == 'probit' else gp.fit_q_softmax_)(X, labels, n_iters=2, start='prior')
    with torch.no_grad():
        fr = Frame(gp)
        a_t, H_t, _ = read_q(gp, fr.T_tt)
        alpha, Q = alpha_Q(fr, a_t, H_t)
        V = ops.matmul(H_t.mT.contiguous(), fr.T[:, fr.n_lt:, :].contiguous()).contiguous()
    y_rows = sites.site_target('bernoulli', labels, C, N)
    fns = {'fused': lambda: gp.loo(X, labels, route='fused'), 'composed': lambda: gp.loo(X, labels, route='composed'),
           'site_moments': lambda: ops.site_moments(fr.theta, fr.z_all, X, alpha, Q, y_rows, None, 'bernoulli', (0,), 0),
           'site_cavity': lambda: ops.site_cavity(fr.theta, fr.z_all, X, alpha, Q, V, y_rows, None, 'bernoulli', (0,), 0)}
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t, outs = {k: [] for k in fns}, {}
    for _ in range(REPS):
        for k, fn in fns.items():
            ms, outs[k] = timed(fn)
            t[k].append(ms)
    f, c = outs['fused'], outs['composed']
    ok = torch.isfinite(f.mu) & torch.isfinite(c.mu)
    rel = lambda a, b: ((a - b)[ok].abs().max() / b[ok].abs().max()).item()
    res = dict(model=name, N=N, D=D, Mt=M, C=C, reps=REPS, fit_iters=fit.n_iters, chunks=ops.site_cavity_chunks(C, M, N, D),
               clock_mhz=clock_mhz(), mean_loo_lpd=f.lpd[torch.isfinite(f.lpd)].mean().item(),
               n_unstable=int(f.n_unstable.sum()), n_unstable_composed=int(c.n_unstable.sum()),
               mu_max_rel_diff=rel(f.mu, c.mu), var_max_rel_diff=rel(f.var, c.var))
    for k, v in t.items():
        res[f'{k}_ms_median'], res[f'{k}_ms_min'] = statistics.median(v), min(v)
    res['composed_over_fused_median'] = res['composed_ms_median'] / res['fused_ms_median']
    res['loo_over_site_moments_median'] = res['fused_ms_median'] / res['site_moments_ms_median']
    res['site_cavity_over_site_moments_median'] = res['site_cavity_ms_median'] / res['site_moments_ms_median']
    print(json.dumps(res), flush=True)
    del gp
