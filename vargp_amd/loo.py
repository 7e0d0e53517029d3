"""Leave-one-out predictive density of the current task's training data from the Gaussian sites of q(u) -- the EP / CVI cavity
(Rasmussen & Williams 5.4.2 for the Gaussian likelihood, where it is the exact LOO of the sparse model; Vehtari et al. 2016 for
latent Gaussian models); not in the reference.  `loo` (VARGP.loo, train_utils.compute_loo) costs about one site pass instead of N
refits, is in the units of VARGP.log_prob and needs no held-out data.

Everything happens at ONE hyper vector, theta = kernel.log_mean, in the whitened coordinates of whitened.py (T, the frozen blocks,
alpha and Q) and with the sites of sites.py.  ASSUMPTION: q(v_t) is a fixed point of the site iteration, i.e. "prior x one
Gaussian site per (output, point)" -- what fit_q_, fit_q_newton_ and fit_q_softmax_ converge to.  With b_n = T k_n, the site of
point n acts on b_n^T v and carries -1/2 lam2_n (b_n^T v)^2 + lam1_n b_n^T v; only v_t is free.  Let

    V = H_t^T T[t, :]   (C, M, Mt),      s_n = |V k_n|^2       (the variance of b_{n,t}^T v_t under q; 0 <= s_n <= var_n)

and r_n = 1 - lam2_n s_n.  Dividing the site out of q(v_t) is a rank-one downdate, and the cavity marginal of f_n is

    mu_-n = (mu_n - s_n lam1_n) / r_n,      var_-n = var_n + lam2_n s_n^2 / r_n

(the frozen tasks' offset b_{n,<}^T a_< cancels in mu_-n).  At a fixed point r_n > 0, since P >= I + lam2_n b b^T; away from one
(a q(u) trained by minibatch steps) r_n can be <= 0: such a point is UNSTABLE, gets NaN moments and a NaN lpd, and is counted.
The LOO lpd of point n is the likelihood's own log predictive density (likelihood.log_prob; csrc/lpd.hip) at the cavity moments.

The sites: Gaussian lam2 = w exp(-obs_log_var), lam1 = lam2 y (independent of q); Bernoulli, Poisson, Student-t those of
ops.site_moments at the current q (the same lam2 >= 0 clamp); softmax those of ops.softmax_sites at (n_f, seed), per (class,
point) -- q factorises over the classes, so all C sites of a point are removed together, each from its own class.

Routes (sites.pick_route): 'fused' up to ops.SITE_MAX_MT inducing points over all tasks -- ONE launch over the data
(ops.site_cavity: marginals, s_n, the likelihood's derivatives and the cavity; K(z, X) and V K never reach memory), or for the
Gaussian and the softmax ops.site_marginals_s with the elementwise cavity step in fp64 torch.  'composed': the same quantities per
tile of N from the gram op and ops.matmul with the cavity arithmetic in fp64 torch; above the limit, on request, and as the
on-device yardstick of the fused kernel."""
from collections import namedtuple

import torch

from . import ops, sites
from .likelihoods import GaussianLikelihood, MulticlassSoftmax
from .whitened import alpha_Q, check_model, read_q

Loo = namedtuple('Loo', 'lpd lpd_out mu var n_unstable stationarity route')
Loo.__doc__ = """lpd (N,): the leave-one-out log predictive density per point (nats; NaN at an unstable point); lpd_out (C, N): each
output's own, or None for the softmax; mu, var (C, N): the cavity moments of f_n; n_unstable (C,) int64: points with r_n <= 0 or a
non-finite cavity, per output; stationarity (C,) float64 or None: |P - (I + A_tt)|_F / |P|_F, the relative distance of the
precision of q(v_t) from "prior + sites" (check=True); route: 'fused' or 'composed'."""


def _check_likelihood(lik, who):
    if not isinstance(lik, (GaussianLikelihood, MulticlassSoftmax)) and getattr(lik, 'kind', None) not in sites.SITE_KINDS:
        raise ValueError(f'{who}: supported likelihoods are GaussianLikelihood, BernoulliLikelihood, PoissonLikelihood, '
                         f'StudentTLikelihood and MulticlassSoftmax, got {type(lik).__name__}')


def check_supported(gp, who='loo'):
    """ValueError unless the cavity applies to the model: ep_var_mean=True, an RBF / Matern / deep-RBF kernel, one of the
    project's likelihoods.  Needs no device."""
    check_model(gp, who, _check_likelihood)
    if isinstance(gp.likelihood, MulticlassSoftmax):
        sites.check_softmax_supported(gp, who)


def cavity_torch(mu, var, s, lam1, lam2):
    """The elementwise cavity step in fp64, rounded once: (C, N) tensors -> (mu_c, var_c fp32 with NaN at the unstable points,
    n_unstable (C,) int64).  A point with lam1 = lam2 = 0 comes out as exactly (mu, var)."""
    mu, var, s, lam1, lam2 = (t.double() for t in (mu, var, s, lam1, lam2))
    r = 1.0 - lam2 * s
    mu_c, var_c = ((mu - s * lam1) / r).float(), (var + lam2 * s * s / r).float()
    bad = ~(r > 0) | ~torch.isfinite(mu_c) | ~torch.isfinite(var_c)
    nan = torch.full_like(mu_c, float('nan'))
    return torch.where(bad, nan, mu_c), torch.where(bad, nan, var_c), bad.sum(-1)


def composed_marginals_s(theta, Z, X, alpha, Q, V, nu2=0, tile=sites.COMPOSED_TILE):
    """ops.site_marginals_s from the per-op kernels, a tile of N at a time (arguments and results alike; any Mt): the gram op and
    ops.matmul for alpha K, Q K and V K."""
    ops.require_device(theta, Z, X, alpha, Q, V)
    (G, Mt, D), N = Z.shape, X.shape[0]
    th = theta.detach().view(1, -1).contiguous()
    g2 = (2.0 * th[0, -1]).exp()
    mu, var, s = (torch.empty(G, N, dtype=torch.float32, device=X.device) for _ in range(3))
    for n0, n1, Xt, _, _ in sites._tiles(X, tile):
        K = sites._gram_tile(th, Z, Xt, nu2)
        mu[:, n0:n1], var[:, n0:n1] = sites._tile_marginals(K, alpha, Q, g2)
        s[:, n0:n1] = ops.matmul(V, K).square().sum(-2)
    return mu, var, s


def composed_site_cavity(theta, Z, X, alpha, Q, V, y, w, kind, extra=(), nu2=0, tile=sites.COMPOSED_TILE):
    """ops.site_cavity from the per-op kernels, a tile of N at a time (arguments and results alike; any Mt): the gram op,
    ops.matmul for alpha K, Q K and V K, ops.lik_nll_bwd with a unit seed for the derivatives, the sites by
    composed_site_moments' formulas and the cavity in fp64 torch."""
    ops.require_device(theta, Z, X, alpha, Q, V, y, w)
    (G, Mt, D), N = Z.shape, X.shape[0]
    th = theta.detach().view(1, -1).contiguous()
    g2 = (2.0 * th[0, -1]).exp()
    seed = torch.ones((), dtype=torch.float32, device=X.device)
    out = ops.SiteCavity(*(torch.empty(G, N, dtype=torch.float32, device=X.device) for _ in range(4)),
                         torch.zeros(G, dtype=torch.int64, device=X.device),
                         *(torch.empty(G, N, dtype=torch.float32, device=X.device) for _ in range(3)))
    gpar = torch.empty(G, dtype=torch.float32, device=X.device) if kind == 'studentt' else None
    for n0, n1, Xt, yt, wt in sites._tiles(X, tile, y, w):
        K = sites._gram_tile(th, Z, Xt, nu2)
        mu, var = sites._tile_marginals(K, alpha, Q, g2)
        s = ops.matmul(V, K).square().sum(-2)
        gmu, gvar = torch.empty_like(mu), torch.empty_like(var)
        ops.lik_nll_bwd(kind, mu.unsqueeze(0), var.unsqueeze(0), ops.lik_target(kind, yt, G, n1 - n0), extra, seed,
                        gmu.unsqueeze(0), gvar.unsqueeze(0), gpar)
        wt = torch.ones_like(mu) if wt is None else wt
        on, zero = wt != 0, torch.zeros_like(mu)
        dvar = -gvar                                                                  # (the seeded gradients are those of -ell)
        l2 = torch.where(on & ~(dvar > 0), wt * (-2.0 * dvar), zero)
        l1 = torch.where(on, wt * (-gmu) + l2 * mu, zero)
        # mu - s w dmu / r = (mu - s lam1) / r without the cancellation of lam2 mu
        gm = torch.where(on, wt.double() * (-gmu).double(), zero.double())
        r = 1.0 - l2.double() * s.double()
        mu_c, var_c = (mu.double() - s.double() * gm / r).float(), (var.double() + l2.double() * s.double().square() / r).float()
        bad = on & (~(r > 0) | ~torch.isfinite(mu_c) | ~torch.isfinite(var_c))
        nan = torch.full_like(mu, float('nan'))
        for dst, src in zip(out, (torch.where(bad, nan, torch.where(on, mu_c, mu)), torch.where(bad, nan, torch.where(on, var_c, var)),
                                  l1, l2, None, mu, var, s)):
            if src is not None:
                dst[:, n0:n1] = src
        out.n_unstable.add_(bad.sum(-1))
    return out


def loo(gp, x, y, weights=None, route=None, check=False, n_f=32, seed=0, tile=sites.COMPOSED_TILE):
    """The leave-one-out log predictive density of the training data x (N, D), y (as the model's fit takes it: fit_q_,
    fit_q_newton_ or fit_q_softmax_) of the current task under the model's CURRENT q(u_t), by the cavity of the module docstring;
    under no_grad, nothing is changed.  weights: the per-point weights the fit used (None, (N,) or (C, N); softmax: None or (N,));
    a point of weight 0 has no site and its cavity is its marginal.  route None / 'fused' / 'composed' as sites.pick_route;
    n_f, seed: the draws of the softmax sites (fit_q_softmax_'s); tile: points per likelihood.log_prob call (and per tile of the
    composed route).  check=True runs the site passes of one iteration as well and fills `stationarity`.  The result is exact LOO
    for a Gaussian likelihood AT a fixed point of the site iteration (after fit_q_), the EP / CVI approximation for the others
    (after fit_q_newton_ / fit_q_softmax_), and only as trustworthy as `stationarity` is small after minibatch training.
    -> Loo(lpd (N,), lpd_out (C, N) or None, mu (C, N), var (C, N), n_unstable (C,), stationarity or None, route)."""
    check_supported(gp)
    lik, tile = gp.likelihood, int(tile)
    if tile < 1:
        raise ValueError(f'loo: tile must be >= 1, got {tile}')
    softmax, gauss = isinstance(lik, MulticlassSoftmax), isinstance(lik, GaussianLikelihood)
    with torch.no_grad():
        pr = sites.problem_for(gp, x, y, weights, route, 'loo', n_f, seed)
        fr, fused = pr.fr, pr.route == 'fused'
        a_t, H_t, L_u = read_q(gp, fr.T_tt)
        alpha, Q = alpha_Q(fr, a_t, H_t)
        V = ops.matmul(H_t.mT.contiguous(), fr.T[:, fr.n_lt:, :].contiguous()).contiguous()
        if softmax or gauss:
            mu, var, s = (ops.site_marginals_s(fr.theta, pr.zf, pr.xf, alpha, Q, V, fr.nu2) if fused else
                          composed_marginals_s(fr.theta, pr.zf, pr.xf, alpha, Q, V, fr.nu2, tile))
            lam1, lam2 = ops.softmax_sites(mu, var, pr.y, pr.w, pr.n_f, pr.seed)[:2] if softmax else pr.gauss_sites()
            mu_c, var_c, n_unstable = cavity_torch(mu, var, s, lam1, lam2)
        else:
            args = (fr.theta, pr.zf, pr.xf, alpha, Q, V, pr.y, pr.w, pr.kind, pr.extra, fr.nu2)
            cav = ops.site_cavity(*args) if fused else composed_site_cavity(*args, tile)
            mu_c, var_c, n_unstable = cav.mu_c, cav.var_c, cav.n_unstable
        parts = [lik.log_prob(mu_c[None, :, n0:n1].contiguous(), var_c[None, :, n0:n1].contiguous(), y[..., n0:n1],
                              per_output=not softmax) for n0 in range(0, pr.N, tile) for n1 in (min(n0 + tile, pr.N),)]
        lpd = torch.cat(parts if softmax else [p[0] for p in parts])
        lpd_out = None if softmax else torch.cat([p[1] for p in parts], dim=-1)
        stationarity = None
        if check:
            P = sites.precision(fr, L_u)
            P_sites = pr.sites(a_t, H_t)[1]
            stationarity = (P - P_sites).square().sum((-2, -1)).sqrt() / P.square().sum((-2, -1)).sqrt()
        return Loo(lpd, lpd_out, mu_c, var_c, n_unstable, stationarity, pr.route)
