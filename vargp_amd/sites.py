"""Natural-gradient fit of q(u) for the non-Gaussian likelihoods with independent outputs -- Bernoulli (probit / logit), Poisson,
Student-t -- by conjugate-computation variational inference (Khan & Lin 2017); not in the reference, whose q(u) is only ever moved
by minibatch gradient steps.  `fit_q_newton_` (VARGP.fit_q_newton_, create_clf / create_reg(q_init='newton')) is the counterpart
of collapsed.fit_q_: a stand-alone, full-batch call under no_grad that overwrites u_mean and u_tril_vec.

Everything happens at ONE hyper vector, theta = kernel.log_mean, in the whitened coordinates of whitened.py's docstring (T, the
frozen tasks' blocks, alpha and Q, A and tc, the KL term and the reader / writer of q(u_t) are defined there).  The new block
starts at the model's current q(u_t): a_t = T_tt u_mean, H_t = T_tt L_u, and is carried in natural parameters P = Sigma_t^-1,
h = P a_t.  One iteration, with k_n = k(z_<=t, x_n) and q(f_n) = N(alpha . k_n, gamma^2 - k_n^T Q k_n):

    mu_n = alpha . k_n,   var_n = max(gamma^2 - k_n^T Q k_n, 0)
    (ell, dmu, dvar) = E_{N(mu_n, var_n)} log p(y_n | f) and its derivatives for (mu_n, var_n)      (csrc/lik.h)
    lam2_n = w_n max(-2 dvar, 0),   lam1_n = w_n dmu + lam2_n mu_n                                  (the Gaussian site of point n)
    c = sum_n lam1_n k_n,   Phi = sum_n lam2_n k_n k_n^T,   A = T Phi T^T,   tc = T c
    P' = (1 - rho) P + rho (I + A_tt),   h' = (1 - rho) h + rho (tc_t - A_{t,<} a_<)
    Sigma_t = P'^-1 = G G^T,   a_t = Sigma_t h'
    bound = sum_n w_n ell - 1/2 (|a_t|^2 + tr Sigma_t - M - logdet Sigma_t)

The first two lines of data terms are ONE fused pass over the data (ops.site_moments, csrc/sites.hip: K(z, X) and the (C, N)
moments never reach memory), Phi a second one (ops.gram_moments with w = lam2).  With rho = 1 and the sites of a Gaussian
likelihood (lam2 = beta, lam1 = beta y) the update is collapsed.fit_q_'s formula; for a log-concave likelihood (Bernoulli,
Poisson) it is Newton's method on the bound.  P' is factored as fit_q_ factors I + beta A_tt: the Cholesky factor of the reversed
matrix, reversed back, so that G is lower triangular and u_tril = L_tt G needs no second factorisation.  Since lam2 >= 0,
P' >= I wherever P >= I.

The data part of a q's bound is the sums[:, 0] of the pass made AT that q, so a candidate's value is known after the next pass.
Backtracking: a candidate whose bound is not finite, or lower than the bound of the q it came from in ANY output, is discarded;
rho is halved for that step and the candidate rebuilt from the same q, at most 8 times; if all fail the fit stops at the last
accepted q.  Every column of the returned trace is therefore non-decreasing.  The fit also stops when the bound summed over the
outputs rises by less than tol |bound|, or after n_iters accepted steps.

CAVEAT (Student-t): the likelihood is not log-concave, d ell / d var can be positive (an outlier), and the clamp lam2 >= 0 then
replaces the Newton step by a Gauss-Newton-like majorisation.  Its fixed point is the stationary point of the bound only when no
point is clamped at convergence: check SiteFit.n_clamped == 0.

Routes: 'fused' as above, for Mt = all inducing points <= ops.SITE_MAX_MT (the K block of all rows lives in LDS).  'composed': the
same quantities per tile of N from the per-op kernels -- the gram op, ops.bgemm, ops.lik_nll_bwd with a unit seed -- and Phi from
ops.gram_moments; taken above the limit, on request (route='composed', or VARGP_SITES_ROUTE=composed in the environment), and as
the on-device yardstick of the fused kernel.  The per-op likelihood entries return their value summed over outputs and points, so
the composed route evaluates ell itself, in fp64 elementwise torch, by the formulas of csrc/lik.h."""
import math
import os
from collections import namedtuple

import torch

from . import ops
from .likelihoods import GaussianLikelihood, MulticlassSoftmax
from .ops import LOWER
from .optim import ascend_, choose_params
from .whitened import Frame, alpha_Q, check_model, kl_standard, mv, read_q, reversed_chol, rows, whiten_moments, write_q_

SiteFit = namedtuple('SiteFit', 'bound n_iters n_rejected n_clamped route')
SiteFit.__doc__ = """bound (n_iters + 1, C) float64 on the host: the variational bound per output at the initial q(u) and after
every accepted step (nats; non-decreasing in every column); n_iters: accepted steps; n_rejected: discarded candidates;
n_clamped: points (over all outputs) whose lam2 was clamped to 0 at the final q(u); route: 'fused' or 'composed'."""

SITE_KINDS = ('bernoulli', 'poisson', 'studentt')
MAX_HALVINGS = 8
COMPOSED_TILE = 8192

# the positive half of numpy.polynomial.hermite.hermgauss(20) and its weights / sqrt(pi) (csrc/lik.h: kGhX, kGhW)
_GH_X = (0.24534070830090124, 0.73747372854539439, 1.2340762153953231, 1.7385377121165861, 2.2549740020892757,
         2.7888060584281305, 3.3478545673832163, 3.9447640401156252, 4.6036824495507442, 5.3874808900112328)
_GH_W = (0.26079306344955488, 0.16173933398399998, 0.061506372063976897, 0.013997837447101022, 0.00183010313108049,
         0.00012882627996192928, 4.402121090230851e-06, 6.127490259982928e-08, 2.4820623623151755e-10, 1.2578006724379234e-13)


def _check_likelihood(lik, who):
    if isinstance(lik, MulticlassSoftmax):
        raise ValueError(f'{who}: MulticlassSoftmax couples the outputs of a point, so it has no independent Gaussian sites; '
                         'its own fit is fit_q_softmax_ (create_clf(q_init="newton_softmax")), or use '
                         'create_clf(likelihood="bernoulli") for a one-vs-rest classifier')
    if isinstance(lik, GaussianLikelihood):
        raise ValueError(f'{who}: for GaussianLikelihood the optimal q(u) has a closed form, use fit_q_')
    if getattr(lik, 'kind', None) not in SITE_KINDS:
        raise ValueError(f'{who}: supported likelihoods are BernoulliLikelihood, PoissonLikelihood and StudentTLikelihood, got '
                         f'{type(lik).__name__}')


def check_supported(gp, who='fit_q_newton_'):
    """ValueError unless the site iteration applies to the model: a Bernoulli, Poisson or Student-t likelihood, ep_var_mean=True,
    an RBF / Matern / deep-RBF kernel.  Needs no device."""
    _Problem.check(gp, who)


def check_damping(damping, who='fit_q_newton_'):
    damping = float(damping)
    if not 0.0 < damping <= 1.0:
        raise ValueError(f'{who}: damping must be in (0, 1], got {damping!r}')
    return damping


def pick_route(route, Mt, who='fit_q_newton_'):
    """route None: VARGP_SITES_ROUTE from the environment if set, else 'fused' up to ops.SITE_MAX_MT inducing points and
    'composed' above.  An explicit 'fused' above the limit is a ValueError."""
    route = route or os.environ.get('VARGP_SITES_ROUTE') or None
    if route not in (None, 'fused', 'composed'):
        raise ValueError(f"{who}: route must be 'fused' or 'composed', got {route!r}")
    if route == 'fused' and Mt > ops.SITE_MAX_MT:
        raise ValueError(f'{who}: the fused pass holds at most {ops.SITE_MAX_MT} inducing points (all tasks), got {Mt}')
    return route or ('fused' if Mt <= ops.SITE_MAX_MT else 'composed')


def site_target(kind, y, C, N):
    """The targets as float32 (C, N) or (N,): Bernoulli int64 class indices (N,) become the one-vs-rest rows (y[n] == c)."""
    if kind == 'bernoulli':
        if y.dtype == torch.int64:
            if tuple(y.shape) != (N,):
                raise ValueError(f'fit_q_newton_: int64 class indices must have shape ({N},), got {tuple(y.shape)}')
            return (y.unsqueeze(0) == torch.arange(C, device=y.device).unsqueeze(1)).to(torch.float32)
        if not (y.dtype.is_floating_point or y.dtype == torch.bool):
            raise TypeError(f'fit_q_newton_: int64 class indices or float / bool 0 / 1 targets, got {y.dtype}')
    return ops.reg_target(y.to(torch.float32), C, N)[0]


def ell_torch(kind, extra, mu, var, y):
    """E_{f ~ N(mu, var)} log p(y | f) elementwise in fp64 torch, by the formulas of csrc/lik.h (the 20-node rule where there is no
    closed form).  mu, var, y broadcastable (C, B); extra as ops.lik_nll_fwd takes it.  Any device."""
    mu, var, y = mu.double(), var.double(), y.double()
    if kind == 'poisson':
        return y * mu - (mu + 0.5 * var).exp() - torch.lgamma(y + 1.0)
    x = torch.tensor(_GH_X, dtype=torch.float64, device=mu.device)
    w = torch.tensor(_GH_W, dtype=torch.float64, device=mu.device)
    pos = var > 0                                                 # (sqrt has no derivative at a variance clamped to 0: that of 1, times 0)
    d = torch.where(pos, (2.0 * torch.where(pos, var, torch.ones_like(var))).sqrt(), torch.zeros_like(var)).unsqueeze(-1) * x
    if kind == 'bernoulli':
        s = (2.0 * y - 1.0).unsqueeze(-1)
        logp = torch.special.log_ndtr if int(extra[0]) == 0 else torch.nn.functional.logsigmoid
        return ((logp(s * (mu.unsqueeze(-1) + d)) + logp(s * (mu.unsqueeze(-1) - d))) * w).sum(-1)
    log_scale, df, lognorm = extra[0].double(), float(extra[1]), float(extra[2])
    inv = ((-2.0 * log_scale).exp() / df).view(-1, 1, 1)
    r0 = (y - mu).unsqueeze(-1)
    el = ((torch.log1p((r0 - d).square() * inv) + torch.log1p((r0 + d).square() * inv)) * w).sum(-1)
    return (lognorm - log_scale).unsqueeze(-1) - 0.5 * (df + 1.0) * el


def _gram_tile(th, Z, Xt, nu2):
    """K (G, Mt, B) = k(Z, Xt) of one tile of points from the gram op; th (1, D+1)."""
    return (ops.rbf_gram(th, Z, Xt, True) if nu2 == 0 else ops.matern_gram(th, Z, Xt, True, 0.5 * nu2))[0]


def _tile_marginals(K, alpha, Q, g2):
    """A tile's K (G, Mt, B) -> (mu = alpha K, var = max(gamma^2 - k Q k, 0)) (G, B), contiguous; Q symmetric, g2 = gamma^2."""
    mu = ops.matmul(alpha.unsqueeze(-2), K).squeeze(-2).contiguous()
    return mu, (g2 - (K * ops.matmul(Q, K)).sum(-2)).clamp_min(0.0).contiguous()


def _tiles(X, tile, y=None, w=None):
    """The tiles of N points: (n0, n1, X[n0:n1], the tile's columns of y and of w, each (N,) or (G, N), or None), contiguous."""
    cols = lambda t, n0, n1: None if t is None else (t[n0:n1] if t.dim() == 1 else t[:, n0:n1]).contiguous()
    for n0 in range(0, X.size(0), tile):
        n1 = min(n0 + tile, X.size(0))
        yield n0, n1, X[n0:n1].contiguous(), cols(y, n0, n1), cols(w, n0, n1)


def composed_site_moments(theta, Z, X, alpha, Q, y, w, kind, extra=(), nu2=0, tile=COMPOSED_TILE):
    """ops.site_moments from the per-op kernels, a tile of N at a time (arguments and results alike; any Mt): the gram op,
    ops.matmul for alpha K and Q K, ops.lik_nll_bwd with a unit seed for the derivatives, ell_torch for the value; c and sums are
    accumulated in fp64 over the tiles."""
    ops.require_device(theta, Z, X, alpha, Q, y, w)
    (G, Mt, D), N = Z.shape, X.shape[0]
    th = theta.detach().view(1, -1).contiguous()
    g2 = (2.0 * th[0, -1]).exp()
    seed = torch.ones((), dtype=torch.float32, device=X.device)
    lam2 = torch.empty(G, N, dtype=torch.float32, device=X.device)
    c = torch.zeros(G, Mt, dtype=torch.float64, device=X.device)
    sums = torch.zeros(G, 4, dtype=torch.float64, device=X.device)
    gpar = torch.empty(G, dtype=torch.float32, device=X.device) if kind == 'studentt' else None
    for n0, n1, Xt, yt, wt in _tiles(X, tile, y, w):
        K = _gram_tile(th, Z, Xt, nu2)
        mu, var = _tile_marginals(K, alpha, Q, g2)
        gmu, gvar = torch.empty_like(mu), torch.empty_like(var)
        ops.lik_nll_bwd(kind, mu.unsqueeze(0), var.unsqueeze(0), ops.lik_target(kind, yt, G, n1 - n0), extra, seed,
                        gmu.unsqueeze(0), gvar.unsqueeze(0), gpar)
        wt = torch.ones_like(mu) if wt is None else wt
        on = wt != 0
        zero = torch.zeros_like(mu)
        dvar = -gvar                                                                  # (the seeded gradients are those of -ell)
        l2 = torch.where(on & ~(dvar > 0), wt * (-2.0 * dvar), zero)
        l1 = torch.where(on, wt * (-gmu) + l2 * mu, zero)
        ell = torch.where(on, wt.double() * ell_torch(kind, extra, mu, var, yt), zero.double())
        lam2[:, n0:n1] = l2
        c += ops.bgemm(K, l1.unsqueeze(-1)).squeeze(-1).double()
        sums += torch.stack([ell.sum(-1), l2.double().sum(-1), (on & (dvar > 0)).double().sum(-1), wt.double().sum(-1)], -1)
    return lam2, c.float(), sums.float()


class _Problem:
    """What the iteration needs of the model and the data, gathered once: theta, the (featurised) inducing points of all tasks
    and inputs, the whitening factors, the frozen tasks' whitened posterior, targets, weights and the likelihood's arguments.
    The class is also the FAMILY -- independent outputs here, the softmax in _SoftmaxProblem: the class attributes and class
    methods are everything in which the two differ, and _bound, _fit_q and _fit_em below are written over a family."""

    who, bound_who, em_who = 'fit_q_newton_', 'site_bound', 'fit_sites_'          # the entry points: fit, bound, EM
    check_likelihood = staticmethod(_check_likelihood)
    max_classes = None
    param_names = ('z', 'kernel', 'lik')                   # what the EM may train; 'lik' where the likelihood has a parameter

    @classmethod
    def check(cls, gp, who, differentiable=False):
        """ValueError unless the family's fit (differentiable: its bound, which refuses a DeepRBFKernel) applies to the model."""
        check_model(gp, who, cls.check_likelihood, deep=f'the feature map needs the gradient of the site pass for its inputs X, '
                    f'which the fused backward does not produce); {cls.who} supports it' if differentiable else None)
        if cls.max_classes is not None and gp.z.size(0) > cls.max_classes:
            raise ValueError(f'{who}: at most {cls.max_classes} classes, got {gp.z.size(0)}')

    @classmethod
    def check_data(cls, who, x, y, weights, fit=False, **draws):
        """The checks of the data and the draws that need no device -> the draws as the problem takes them (here: none)."""
        return {}

    @classmethod
    def operands(cls, lik, y, weights, C, N, who, graph=False):
        """What follows (alpha, Q) in the argument list of the family's passes: (targets, weights, kind, extra).  graph: the
        likelihood's own parameter stays on the autograd graph (the bound); else everything is detached (the fit)."""
        if graph:
            own = lik.ext_param()
            extra = (() if own is None else (own.to(torch.float32),)) + tuple(lik._consts())
        else:
            extra = tuple(t.detach() if torch.is_tensor(t) else t for t in lik._extra())
        return site_target(lik.kind, y.detach(), C, N), None if weights is None else rows(weights, C, N), lik.kind, extra

    @staticmethod
    def diff_pass(route):
        """The data term of the bound on the autograd graph: (theta, Z, X, alpha, Q, *operands, nu2) -> value."""
        return ops.site_bound_diff if route == 'fused' else composed_site_bound

    @staticmethod
    def reduce_kl(kl):
        """KL(q(v_t) || N(0, I)) (C,) as the bound holds it: one entry per output."""
        return kl

    def __init__(self, gp, x, y, weights, route, who=None):
        self.who = who or self.who
        self.fr = fr = Frame(gp)
        self.C, self.M, self.N = fr.C, fr.M, x.size(0)
        self.route = pick_route(route, fr.Mt, self.who)
        self._targets(gp.likelihood, y, weights)
        self.zf, self.xf = fr.operands(x.detach().contiguous())
        self.eye = torch.eye(fr.M, dtype=torch.float64, device=x.device)

    def _targets(self, lik, y, weights):
        """The likelihood's arguments, the targets and the weights as the data passes take them."""
        self.y, self.w, self.kind, self.extra = self.operands(lik, y, weights, self.C, self.N, self.who)

    def _passes(self, alpha, Q):
        """The passes over the data at q(f_n) = N(alpha . k_n, gamma^2 - k_n^T Q k_n): -> (Phi (C, Mt, Mt), c (C, Mt), the data
        term of the bound float64, clamped points)."""
        pass_ = ops.site_moments if self.route == 'fused' else composed_site_moments
        lam2, c, sums = pass_(self.fr.theta, self.zf, self.xf, alpha, Q, self.y, self.w, self.kind, self.extra, self.fr.nu2)
        Phi = ops.gram_moments(self.fr.theta, self.zf, self.xf, lam2, lam2, self.fr.nu2)[0]
        return Phi, c, sums[:, 0].double(), sums[:, 2]

    def bound(self, data, kl):
        """The bound as the trace holds it, from the data term and KL(q(v_t) || N(0, I)) (C,)."""
        return data - self.reduce_kl(kl)

    def sites(self, a_t, H_t):
        """The passes over the data at q(v_t) = N(a_t, H_t H_t^T): -> (the data term of the bound, float64, I + A_tt,
        tc_t - A_{t,<} a_<, clamped points)."""
        fr, n_lt = self.fr, self.fr.n_lt
        Phi, c, data, clamped = self._passes(*alpha_Q(fr, a_t, H_t))
        A, tc = whiten_moments(fr.T, Phi, c)
        P_new = self.eye + A[:, n_lt:, n_lt:]
        h_new = tc[:, n_lt:] - mv(A[:, n_lt:, :n_lt], fr.frozen[0])
        return data, P_new, h_new, clamped

    def from_natural(self, P, h):
        """Sigma_t = P^-1 = G G^T with G lower triangular (the Cholesky factor of the reversed P, reversed back, as fit_q_ factors
        I + beta A_tt) -> (a_t = Sigma_t h, G float32, KL(q(v_t) || N(0, I)) (C,))."""
        Lr, G = reversed_chol(P)
        G64 = G.double().tril()
        a_t = mv(G64, mv(G64.mT, h))
        logdet_sigma = -2.0 * Lr.diagonal(dim1=-2, dim2=-1).double().log().sum(-1)
        kl = 0.5 * (a_t.square().sum(-1) + G64.square().sum((-2, -1)) - self.M - logdet_sigma)
        return a_t, G.tril(), kl


def whitened_q(gp):
    """The model's current q(u_t) in whitened coordinates at the current parameters: -> (a_t = T_tt u_mean (C, M) float64,
    H_t = T_tt L_u (C, M, M) float32, lower triangular), detached."""
    ops.require_device(gp.z)
    with torch.no_grad():
        return read_q(gp, Frame(gp).T_tt)[:2]


def set_whitened_q_(gp, a_t, H_t):
    """Write q(v_t) = N(a_t, H_t H_t^T) as u_mean = L_tt a_t, u_tril = L_tt H_t at the CURRENT parameters into u_mean /
    u_tril_vec: what keeps q fixed in whitened coordinates after inducing points or hyper-parameters have moved."""
    ops.require_device(gp.z, a_t, H_t)
    with torch.no_grad():
        write_q_(gp, Frame(gp).L_tt, a_t.double(), H_t.float().contiguous())


def fit_q_newton_(gp, x, y, n_iters=20, damping=1.0, tol=1e-6, weights=None, route=None, start='current'):
    """Fit q(u_t) of the VARGP model `gp` (Bernoulli, Poisson or Student-t likelihood) to the data x (N, D), y as loss() takes it
    ((N,) or (C, N); Bernoulli: int64 class indices (N,) read one-vs-rest, or float / bool 0 / 1 targets), by the natural-gradient
    site iteration of the module docstring, started at the model's current q(u_t); in place and under no_grad.  At most n_iters
    accepted steps of length damping in (0, 1] (halved while a candidate lowers the bound), until the summed bound rises by less
    than tol |bound|.  weights None, (N,) or (C, N), >= 0: per-point weights of the log-likelihood.  First-task models and models
    with prev_params alike; hyper-parameters, inducing points and the likelihood's own parameters are read, not changed.
    route: None (the fused pass up to ops.SITE_MAX_MT inducing points, the composed one above; VARGP_SITES_ROUTE overrides),
    'fused' or 'composed'.  start: 'current' (the model's u_mean / u_tril_vec) or 'prior' (q(u_t) = p(u_t | u_<): a_t = 0, H_t = I;
    the model's q(u_t) is then not read).  The default start of a VARGP model (u_tril = 1.31 I in the space of u) is a WIDE q in
    function space; a Poisson likelihood, whose expected log-likelihood holds exp(mu + var / 2), can be far too steep there for
    any damped step to be accepted -- start such a model at the prior.  -> SiteFit(bound (n_iters + 1, C) float64 on the host, n_iters, n_rejected, n_clamped, route)."""
    return _fit_q(_Problem, gp, x, y, n_iters, damping, tol, weights, route, start)


def _fit_q(family, gp, x, y, n_iters, damping, tol, weights, route, start, **draws):
    """The prologue of the family's fit: the model, the loop arguments, the data and the draws, the device; then _fit."""
    family.check(gp, family.who)
    damping, n_iters = _check_loop_args(family.who, damping, n_iters, start)
    draws = family.check_data(family.who, x, y, weights, fit=True, **draws)
    ops.require_device(gp.z, x, y, weights)
    with torch.no_grad():
        return _fit(gp, family(gp, x, y, weights, route, **draws), n_iters, damping, tol, start)


def _check_loop_args(who, damping, n_iters, start):
    damping = check_damping(damping, who)
    n_iters = int(n_iters)
    if n_iters < 0:
        raise ValueError(f'{who}: n_iters must be >= 0, got {n_iters}')
    if start not in ('current', 'prior'):
        raise ValueError(f"{who}: start must be 'current' or 'prior', got {start!r}")
    return damping, n_iters


def precision(fr, L_u):
    """P = (H_t H_t^T)^-1 (C, M, M) float64, symmetrised, of the model's q(u_t) = N(., L_u L_u^T) in whitened coordinates:
    H_t^-1 = L_u^-1 L_tt."""
    T_u = ops.chol_inv(ops.bgemm(L_u, L_u.mT), 0.0)[1]
    H_inv = ops.bgemm(T_u, fr.L_tt, triA=LOWER, triB=LOWER).tril()
    P = ops.bgemm(H_inv.mT, H_inv).double()
    return 0.5 * (P + P.mT)


def _fit(gp, pr, n_iters, damping, tol, start):
    """The iteration of the module docstring on the problem `pr` (its passes over the data, its form of the bound), from `start`
    with backtracking; writes the last accepted q(u_t) into gp.  Under no_grad.  -> SiteFit"""
    M, dev = pr.M, pr.fr.theta.device
    if start == 'prior':
        a_t = torch.zeros(pr.C, M, dtype=torch.float64, device=dev)
        H_t = torch.eye(M, dtype=torch.float32, device=dev).expand(pr.C, M, M).contiguous()
        P, h, kl = pr.eye.expand(pr.C, M, M), torch.zeros_like(a_t), torch.zeros(pr.C, dtype=torch.float64, device=dev)
    else:
        # the model's q(u_t) in whitened coordinates and natural parameters: H_t^-1 = L_u^-1 L_tt
        a_t, H_t, L_u = read_q(gp, pr.fr.T_tt)
        P = precision(pr.fr, L_u)
        h = mv(P, a_t)
        kl = kl_standard(a_t, H_t)

    data, P_new, h_new, clamped = pr.sites(a_t, H_t)
    bound = pr.bound(data, kl).cpu()
    if not bool(torch.isfinite(bound).all()):
        raise FloatingPointError(f'{pr.who}: the bound is not finite at the initial q(u): {bound.tolist()}')
    trace, n_rejected, changed = [bound], 0, start == 'prior'
    while len(trace) - 1 < n_iters:
        rho, accepted = damping, None
        for _ in range(MAX_HALVINGS + 1):
            P_c, h_c = (1.0 - rho) * P + rho * P_new, (1.0 - rho) * h + rho * h_new
            a_c, G_c, kl_c = pr.from_natural(P_c, h_c)
            data_c, P_next, h_next, clamped_c = pr.sites(a_c, G_c)
            bound_c = pr.bound(data_c, kl_c).cpu()
            if bool(torch.isfinite(bound_c).all()) and bool((bound_c >= trace[-1]).all()):
                accepted = (P_c, h_c, a_c, G_c, P_next, h_next, clamped_c)
                break
            n_rejected += 1
            rho *= 0.5
        if accepted is None:
            break
        P, h, a_t, H_t, P_new, h_new, clamped = accepted
        trace.append(bound_c)
        changed = True
        if (trace[-1].sum() - trace[-2].sum()).item() < tol * abs(trace[-1].sum().item()):
            break

    if changed:
        write_q_(gp, pr.fr.L_tt, a_t, H_t)
    n_clamped = int(round(clamped.double().sum().item()))
    return SiteFit(torch.stack(trace), len(trace) - 1, n_rejected, n_clamped, pr.route)


# -- the softmax: coupled outputs, one Gaussian site per (class, point) all the same --------------------------------------------------
# q factorises over the classes, so conjugate-computation VI still gives one Gaussian site per (class, point); the coupling is
# only in how the site parameters are COMPUTED: all C marginals of a point enter one expectation over p = softmax(f_n),
# f_n ~ N(mu_n, diag(var_n)):
#     ell_n = E log p_{y_n} = mu_{y_n, n} - E logsumexp(f_n)
#     d ell / d mu_c = [y_n = c] - E p_c (Bonnet),   d ell / d var_c = -1/2 E[p_c (1 - p_c)] <= 0 (Price): nothing is ever clamped
#     lam2_cn = w_n E[p_c (1 - p_c)],   lam1_cn = w_n ([y_n = c] - E p_c) + lam2_cn mu_cn
# Everything after that is the iteration of the module docstring, per class.  The expectations are Monte-Carlo means over n_f draws
# per point, as the softmax nll takes them, with noise FIXED for the whole fit (common random numbers: a counter-based stream keyed
# by `seed`, generated inside the kernel), so the bound is a deterministic function of q.  The data term is joint over the
# classes: a candidate is accepted on the SUMMED bound, and the trace has one column.
# One iteration is three launches-with-reduce over the data: ops.site_marginals (site_moments' kernel stopped after mu and var),
# ops.softmax_sites, ops.gram_moments_v(w=lam2, v=lam1) -- v a weight vector of its own because lam1 / lam2 is not representable:
# lam2 underflows to 0 exactly at the confidently MISCLASSIFIED points, where lam1 ~ 1 matters most.
# CAVEAT: lam1 and lam2 are unbiased Bonnet / Price estimates of the derivatives of the exact ell; they are NOT the exact
# derivatives of its n_f-sample estimate (whose derivative for var_c holds eps / sqrt(var) terms).  Near the optimum a full step
# can therefore lower the ESTIMATED bound, by about 1e-5 relative; the fit then ends by rejection (all halvings fail) rather than
# by tol, at the last accepted q.
def _check_softmax_likelihood(lik, who):
    if not isinstance(lik, MulticlassSoftmax):
        raise ValueError(f'{who}: supported for MulticlassSoftmax only, got {type(lik).__name__}; the likelihoods with '
                         'independent outputs have fit_q_newton_ (q_init="newton"), GaussianLikelihood has fit_q_')


def _class_indices(who, y, N):
    if y.dtype != torch.int64 or tuple(y.shape) != (N,):
        raise ValueError(f'{who}: y must be int64 class indices of shape ({N},), got {y.dtype} {tuple(y.shape)}')
    return y


def check_softmax_supported(gp, who='fit_q_softmax_'):
    """ValueError unless the softmax site iteration applies to the model: MulticlassSoftmax, ep_var_mean=True, an RBF / Matern /
    deep-RBF kernel.  Needs no device."""
    _SoftmaxProblem.check(gp, who)


def composed_softmax_marginals(theta, Z, X, alpha, Q, nu2=0, tile=COMPOSED_TILE):
    """ops.site_marginals from the per-op kernels, a tile of N at a time (arguments and results alike; any Mt): the gram op and
    ops.matmul for alpha K and Q K."""
    ops.require_device(theta, Z, X, alpha, Q)
    (G, Mt, D), N = Z.shape, X.shape[0]
    th = theta.detach().view(1, -1).contiguous()
    g2 = (2.0 * th[0, -1]).exp()
    mu = torch.empty(G, N, dtype=torch.float32, device=X.device)
    var = torch.empty(G, N, dtype=torch.float32, device=X.device)
    for n0, n1, Xt, _, _ in _tiles(X, tile):
        mu[:, n0:n1], var[:, n0:n1] = _tile_marginals(_gram_tile(th, Z, Xt, nu2), alpha, Q, g2)
    return mu, var


def composed_softmax_sites(mu, var, y, w, eps):
    """ops.softmax_sites in plain fp32 elementwise torch on the device, with explicit eps (n_f, C, N) (arguments and results
    alike; the sums in fp64): the on-device yardstick of the kernel."""
    ops.require_device(mu, var, y, w, eps)
    C, N = mu.shape
    f = mu + var.sqrt() * eps                                                         # (F, C, N)
    m = f.max(-2, keepdim=True).values
    e = (f - m).exp()
    s = e.sum(-2, keepdim=True)
    p = e / s
    lse = (m + s.log()).squeeze(-2).mean(0)                                           # (N,)
    Ep, Ev = p.mean(0), (p * (1.0 - p)).mean(0)
    wt = torch.ones(N, dtype=torch.float32, device=mu.device) if w is None else w
    on = wt != 0
    hot = (y.unsqueeze(0) == torch.arange(C, device=y.device).unsqueeze(1)).to(torch.float32)
    zero = torch.zeros_like(mu)
    lam2 = torch.where(on, wt * Ev, zero)
    lam1 = torch.where(on, wt * (hot - Ep) + lam2 * mu, zero)
    ell = torch.where(on, wt.double() * ((mu * hot).sum(0) - lse).double(), torch.zeros(N, dtype=torch.float64, device=mu.device))
    sums = torch.stack([ell.sum(), lam2.double().sum(), on.double().sum(), wt.double().sum()])
    return lam1, lam2, sums.float()


class _SoftmaxProblem(_Problem):
    """_Problem with the softmax's three passes and its joint data term: the softmax family."""
    who, bound_who, em_who = 'fit_q_softmax_', 'softmax_site_bound', 'fit_softmax_sites_'
    check_likelihood = staticmethod(_check_softmax_likelihood)
    max_classes = ops.SOFTMAX_SITE_MAX_C
    param_names = ('z', 'kernel')                          # the softmax has no parameter

    @classmethod
    def check_data(cls, who, x, y, weights, fit=False, n_f=32, seed=0):
        """n_f in [1, 65535], y int64 (N,), weights None or (N,).  fit: fit_q_softmax_, which checks y with its targets (on the
        device) and words the weights' refusal at more length."""
        N, n_f = x.size(0), int(n_f)
        if not 1 <= n_f <= 65535:
            raise ValueError(f'{who}: n_f must be in [1, 65535], got {n_f}')
        if not fit:
            _class_indices(who, y, N)
        if weights is not None and tuple(weights.shape) != (N,):
            shared = ' (the classes of a point share one likelihood term)' if fit else ''
            raise ValueError(f'{who}: weights must have shape ({N},): one weight per point{shared}, got {tuple(weights.shape)}')
        return dict(n_f=n_f, seed=seed)

    @classmethod
    def operands(cls, lik, y, weights, C, N, who, graph=False):
        """(class indices, weights (N,)): what follows (alpha, Q) in the softmax passes, before the draws."""
        return _class_indices(who, y.detach(), N).contiguous(), None if weights is None else weights.detach().to(torch.float32).contiguous()

    @staticmethod
    def diff_pass(route):
        return ops.softmax_site_bound_diff if route == 'fused' else composed_softmax_site_bound

    @staticmethod
    def reduce_kl(kl):
        """Summed over the classes: the data term is joint."""
        return kl.sum(-1, keepdim=True)

    def __init__(self, gp, x, y, weights, route, n_f=32, seed=0, who=None):
        self.n_f, self.seed = n_f, int(seed)
        super().__init__(gp, x, y, weights, route, who)

    def _targets(self, lik, y, weights):
        self.y, self.w = self.operands(lik, y, weights, self.C, self.N, self.who)

    def _passes(self, alpha, Q):
        marginals = ops.site_marginals if self.route == 'fused' else composed_softmax_marginals
        mu, var = marginals(self.fr.theta, self.zf, self.xf, alpha, Q, self.fr.nu2)
        lam1, lam2, sums = ops.softmax_sites(mu, var, self.y, self.w, self.n_f, self.seed)
        Phi, c, _ = ops.gram_moments_v(self.fr.theta, self.zf, self.xf, lam2, lam1, self.fr.nu2)
        return Phi, c, sums[:1].double(), torch.zeros((), device=mu.device)


def fit_q_softmax_(gp, x, y, n_iters=20, damping=1.0, tol=1e-6, weights=None, route=None, start='current', n_f=32, seed=0):
    """fit_q_newton_ for the model the project exists for: fit q(u_t) of a MulticlassSoftmax VARGP model to the data x (N, D), y
    (N,) int64 class indices, by the natural-gradient site iteration of the module docstring with the softmax sites of the comment
    above; in place and under no_grad.  The expectations over the softmax are means over n_f draws per point whose noise is fixed
    by `seed` for the whole fit, so the bound is a deterministic function of q and the trace never falls.  At most n_iters accepted
    steps of length damping in (0, 1] (halved while a candidate lowers the SUMMED bound -- the data term is joint over the
    classes), until it rises by less than tol |bound|.  weights None or (N,), >= 0.  First-task models and models with
    prev_params; RBF, Matern and deep-RBF kernels; ep_var_mean=True.  route: None ('fused' up to ops.SITE_MAX_MT inducing points
    over all tasks, 'composed' above; VARGP_SITES_ROUTE overrides), 'fused' or 'composed' (the marginals from the gram op and
    ops.bgemm a tile of N at a time; the other two passes have no limit).  start: 'current' or 'prior', as fit_q_newton_.
    CAVEAT: lam1 and lam2 are unbiased Bonnet / Price estimates, not the exact derivatives of the n_f-sample estimate of the
    expected log-likelihood: near the optimum a full step can lower the estimated bound by about 1e-5 relative, and the fit then
    ends by rejection rather than by tol, at the last accepted q.
    -> SiteFit(bound (n_iters + 1, 1) float64 on the host: the summed bound, non-decreasing; n_iters; n_rejected; n_clamped = 0
    always (d ell / d var <= 0); route)."""
    return _fit_q(_SoftmaxProblem, gp, x, y, n_iters, damping, tol, weights, route, start, n_f=n_f, seed=seed)


class _GaussProblem(_Problem):
    """_Problem with the sites of a Gaussian likelihood, which do not depend on q: lam2 = w / sigma^2, lam1 = lam2 y.  Its fit is
    collapsed.fit_q_; the problem serves loo.py."""

    def gauss_sites(self):
        beta = (-self.extra[0].double()).exp().unsqueeze(-1)
        lam2 = beta.expand(self.C, self.N) if self.w is None else self.w.double() * beta
        return lam2 * rows(self.y, self.C, self.N).double(), lam2

    def _passes(self, alpha, Q):
        lam1, lam2 = (t.float().contiguous() for t in self.gauss_sites())
        Phi, c, _ = ops.gram_moments_v(self.fr.theta, self.zf, self.xf, lam2, lam1, self.fr.nu2)
        zero = torch.zeros(self.C, dtype=torch.float64, device=lam2.device)
        return Phi, c, zero, zero


def problem_for(gp, x, y, weights, route, who, n_f=32, seed=0):
    """The problem of the model's family -- softmax, Gaussian or independent non-Gaussian outputs -- for the caller `who`, with
    the family's checks of the data and the draws (n_f, seed: the softmax's) made first and the operands required on a device."""
    lik = gp.likelihood
    family = _SoftmaxProblem if isinstance(lik, MulticlassSoftmax) else _GaussProblem if isinstance(lik, GaussianLikelihood) else _Problem
    draws = family.check_data(who, x, y, weights, n_f=n_f, seed=seed)
    ops.require_device(gp.z, x, y, weights)
    return family(gp, x, y, weights, route, who=who, **draws)


# -- the site bound on the autograd graph: variational EM ----------------------------------------------------------------------------
# With q(v_t) = N(a_t, H_t H_t^T) held FIXED in whitened coordinates, the bound of the module docstring is a function of the
# inducing points, theta = kernel.log_mean and the likelihood's own parameter through alpha = T^T a, Q = T^T (I - H H^T) T and
# k_n alone (the KL term is a constant), and d bound / d (alpha, Q, K) are sums over the points:
#     gm_n = s w_n d ell_n / d mu,   gv_n = s w_n d ell_n / d var [gamma^2 - k_n^T Q k_n > 0]      (the TRUE signed d ell / d var)
#     galpha = sum_n gm_n k_n,   gQ = -sum_n gv_n k_n k_n^T,   gK[:, n] = gm_n alpha - 2 gv_n Q k_n
# ops.site_bound_diff is that function with ONE fused backward pass (csrc/sites.hip: vargp_site_bound_bwd; gQ by ops.gram_moments
# with w = gv); the frozen tasks' a_i = T_ii m_i, H_i = T_ii Lu_i and T itself are differentiated by the per-op nodes
# (ops.chol_inv, ops.matmul): whitened.py.  fit_sites_ alternates fit_q_newton_ (E-step) with a few Yogi
# steps on the bound (M-step); by the envelope theorem the partial gradient at the fixed whitened q IS the gradient of the
# re-converged bound at a converged E-step (tests/test_site_bound_host.py).
EMFit = namedtuple('EMFit', 'bound n_rounds n_newton stopped')
EMFit.__doc__ = """bound (n_rounds + 1, C) float64 on the host: the bound per output after every E-step (its sum over the outputs
is non-decreasing); n_rounds: completed rounds (M-step + E-step); n_newton: accepted Newton steps over all E-steps; stopped:
'rounds' (all rounds done) or 'm_step' (an M-step lowered the bound and was undone)."""


def check_differentiable(gp, who):
    """check_supported, and exactly RBFKernel or MaternKernel: the bound's gradient for a DeepRBFKernel needs the gradient of the
    site pass for its inputs X (the feature map), which the fused backward does not produce."""
    _Problem.check(gp, who, differentiable=True)


def _tile_value(leaves, Xt, yt, wt, kind, extra, nu2):
    """sum_n w_n ell_n (G,) float64 of one tile of points from the differentiable per-op nodes: the gram op, ops.matmul, and
    ell_torch in fp64.  leaves: theta, Z, alpha, Q and, for Student-t, log_scale."""
    theta, Z, alpha, Q, *log_scale = leaves
    mu, var = _tile_marginals(_gram_tile(theta.view(1, -1), Z, Xt, nu2), alpha, 0.5 * (Q + Q.mT), (2.0 * theta[-1]).exp())
    ell = ell_torch(kind, tuple(log_scale) + tuple(extra[1:]) if log_scale else extra, mu, var, yt)
    if wt is None:
        return ell.sum(-1)
    return torch.where(wt != 0, wt.double() * ell, torch.zeros_like(ell)).sum(-1)


class _ComposedBound(torch.autograd.Function):
    """The composed route of both differentiable bounds, for any Mt, a tile of N at a time: the forward adds the tiles' values
    tile_value(leaves, Xt, yt, wt, *per_tile(n0, n1)) in fp64 under no_grad; the backward revisits the same tiles, rebuilds each
    tile's graph from the per-op nodes and accumulates the gradients of the leaves in fp64 -- memory O(Mt x tile).  per_tile: the
    tile's further arguments (the likelihood's constants; the tile's slice of the softmax noise); n_out: the size of the value."""
    @staticmethod
    def forward(ctx, tile_value, per_tile, n_out, tile, X, y, w, *leaves):
        ctx.save_for_backward(X, y, w, *leaves)
        ctx.cfg = (tile_value, per_tile, tile)
        value = torch.zeros(n_out, dtype=torch.float64, device=X.device)
        for n0, n1, Xt, yt, wt in _tiles(X, tile, y, w):
            value += tile_value(leaves, Xt, yt, wt, *per_tile(n0, n1))
        return value

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        X, y, w, *saved = ctx.saved_tensors
        tile_value, per_tile, tile = ctx.cfg
        leaves = [t.detach().clone().requires_grad_(True) for t in saved]
        acc = [torch.zeros(t.shape, dtype=torch.float64, device=t.device) for t in leaves]
        with torch.enable_grad():
            for n0, n1, Xt, yt, wt in _tiles(X, tile, y, w):
                val = tile_value(leaves, Xt, yt, wt, *per_tile(n0, n1))
                for a, g in zip(acc, torch.autograd.grad((val * gout.double()).sum(), leaves)):
                    a += g.double()
        return (None,) * 7 + tuple(a.to(t.dtype) for a, t in zip(acc, leaves))


def composed_site_bound(theta, Z, X, alpha, Q, y, w, kind, extra=(), nu2=0, tile=COMPOSED_TILE):
    """ops.site_bound_diff from the per-op kernels (arguments alike, any Mt; value (G,) float64): the route above
    ops.SITE_MAX_MT inducing points and the on-device yardstick of the fused backward."""
    ops.require_device(theta, Z, X, alpha, Q, y, w)
    ops.refuse_grad('composed_site_bound', ops.SITE_BOUND_GRADS, X=X, y=y, w=w)
    consts = (kind, tuple(extra), int(nu2))
    return _ComposedBound.apply(_tile_value, lambda n0, n1: consts, Z.size(0), int(tile), X, y, w, theta, Z, alpha, Q,
                                *((extra[0],) if kind == 'studentt' else ()))


def _bound(family, gp, x, y, weights, q, route, who, **draws):
    """The family's bound on the autograd graph: data term - KL.  The nodes are created in this order -- Frame, whitened_q, the
    likelihood's operands, alpha_Q, the data pass, kl_standard -- and autograd adds gradients in the reverse of it (whitened.py)."""
    family.check(gp, who, differentiable=True)
    draws = family.check_data(who, x, y, weights, **draws)
    ops.require_device(gp.z, x, y, weights)
    fr = Frame(gp)
    route = pick_route(route, fr.Mt, who)
    a_t, H_t = whitened_q(gp) if q is None else (q[0].detach().double(), q[1].detach().float())
    operands = family.operands(gp.likelihood, y, weights, fr.C, x.size(0), who, graph=True)
    data = family.diff_pass(route)(fr.theta, fr.z_all, x.detach().contiguous(), *alpha_Q(fr, a_t, H_t), *operands, nu2=fr.nu2, **draws)
    return data.double() - family.reduce_kl(kl_standard(a_t, H_t))


def site_bound(gp, x, y, weights=None, q=None, route=None):
    """The variational bound of the data x (N, D), y (as fit_q_newton_ takes it) per output, (C,) float64: data term -
    KL(q(v_t) || N(0, I)), ON THE AUTOGRAD GRAPH of gp.z, gp.kernel.log_mean and, for Student-t, gp.likelihood.log_scale.
    q = (a_t (C, M), H_t (C, M, M) lower) is q(u_t) in whitened coordinates and a CONSTANT; None: whitened_q(gp), the model's own,
    with which the value is fit_q_newton_(n_iters=0).bound[0].  The frozen tasks' inducing points and q(u) are constants; their
    whitened moments depend on theta through the whitening and are differentiated.  x, y and weights get no gradient.  One fused
    pass over the data forward and one backward plus one ops.gram_moments call; K(z, x) is never stored (route 'fused', up to
    ops.SITE_MAX_MT inducing points over all tasks; 'composed' above it or on request: per-op kernels, a tile of N at a time).
    Bernoulli, Poisson or Student-t likelihood, ep_var_mean=True, exactly RBFKernel or MaternKernel; a DeepRBFKernel is refused
    (ValueError).  The hyper-prior (kl_hypers) is NOT part of the bound."""
    return _bound(_Problem, gp, x, y, weights, q, route, 'site_bound')


def fit_sites_(gp, x, y, n_rounds=5, m_steps=20, lr=1e-2, params=None, newton_iters=20, damping=1.0, tol=1e-6, weights=None,
               route=None, start='current'):
    """Variational EM on the site bound, full batch and in place.  Every round: E-step fit_q_newton_(n_iters=newton_iters,
    damping, tol; the first from `start`, the later ones from the current q); M-step m_steps steps of the project's Yogi
    (optim.py, step lr) on -sum_c site_bound over the chosen subset `params` of {'z': gp.z, 'kernel': gp.kernel.log_mean, 'lik':
    the likelihood's own parameter (Student-t log_scale)} with q held at the E-step's whitened (a_t, H_t), then
    set_whitened_q_.  A last E-step ends the fit.  params None: ('z', 'kernel'), and 'lik' where the likelihood has a
    parameter; 'lik' on a likelihood without one is a ValueError.  An M-step after which the summed bound is lower than before
    it is undone (parameters and q restored), stopped = 'm_step', and the loop ends: the summed trace never falls.  The
    objective is the bound alone: the hyper-prior (kl_hypers) is NOT in it, so this is maximum likelihood (type II) for the
    hyper-parameters, not the MAP / variational treatment of VARGP.loss.  -> EMFit(bound (n_rounds + 1, C) float64 on the
    host, n_rounds, n_newton, stopped)."""
    return _fit_em(_Problem, gp, x, y, n_rounds, m_steps, lr, params, newton_iters, damping, tol, weights, route, start)


def _fit_em(family, gp, x, y, n_rounds, m_steps, lr, params, newton_iters, damping, tol, weights, route, start, **draws):
    """The prologue of the family's EM: the model, the trainable subset, the loop arguments, the data and the draws, the device;
    then _em on the family's fit and bound.  A family whose param_names hold 'lik' refuses it after the subset is chosen, where
    the likelihood has no parameter; one without 'lik' refuses it at once."""
    who, lik = family.em_who, gp.likelihood
    family.check(gp, who, differentiable=True)
    named = dict(z=gp.z, kernel=gp.kernel.log_mean, lik=lik.ext_param() if 'lik' in family.param_names else None)
    params = tuple(k for k, t in named.items() if t is not None) if params is None else tuple(params)
    named = {k: named[k] for k in family.param_names}
    no_lik = 'lik' in params and named.get('lik') is None and ValueError(f"{who}: params names 'lik', but {type(lik).__name__} has "
                                                                         'no parameter')
    if no_lik and 'lik' not in named:
        raise no_lik
    chosen = choose_params(who, named, params)
    if no_lik:
        raise no_lik
    damping, n_rounds, m_steps = _check_em_args(who, damping, n_rounds, m_steps)
    draws = family.check_data(who, x, y, weights, **draws)
    ops.require_device(gp.z, x, y, weights)
    e_step = lambda st: _fit_q(family, gp, x, y, newton_iters, damping, tol, weights, route, st, **draws)
    bound_at = lambda q: _bound(family, gp, x, y, weights, q, route, family.bound_who, **draws)
    return _em(gp, chosen, e_step, bound_at, start, n_rounds, m_steps, lr)


def _check_em_args(who, damping, n_rounds, m_steps):
    damping = check_damping(damping, who)
    n_rounds, m_steps = int(n_rounds), int(m_steps)
    if n_rounds < 0 or m_steps < 0:
        raise ValueError(f'{who}: n_rounds and m_steps must be >= 0, got {n_rounds}, {m_steps}')
    return damping, n_rounds, m_steps


def _em(gp, chosen, e_step, bound_at, start, n_rounds, m_steps, lr):
    """The round loop both EM fits share: e_step(start) -> a SiteFit (the first from `start`, the later ones from 'current');
    bound_at(q) -> the bound on the autograd graph of `chosen` with q(v_t) held at the whitened q; the undo rule of fit_sites_'
    docstring.  -> EMFit"""
    fit = e_step(start)
    trace, n_newton, stopped, done = [fit.bound[-1]], fit.n_iters, 'rounds', 0
    for _ in range(n_rounds):
        q = whitened_q(gp)
        keep = [t.detach().clone() for t in chosen + [gp.u_mean, gp.u_tril_vec]]

        def undo():
            with torch.no_grad():
                for t, k in zip(chosen + [gp.u_mean, gp.u_tril_vec], keep):
                    t.copy_(k)

        before = ascend_(lambda: bound_at(q), chosen, m_steps, lr)
        if m_steps:
            with torch.no_grad():
                after = bound_at(q).sum()
            if not bool(after >= before[0].sum()):
                undo()
                stopped = 'm_step'
                break
            set_whitened_q_(gp, *q)
        fit = e_step('current')
        if not bool(fit.bound[-1].sum() >= trace[-1].sum()):       # (rounding between the M-step's bound and the E-step's own)
            undo()
            stopped = 'm_step'
            break
        trace.append(fit.bound[-1])
        n_newton += fit.n_iters
        done += 1
    return EMFit(torch.stack(trace), done, n_newton, stopped)


# -- the softmax site bound on the autograd graph: variational EM for MulticlassSoftmax ---------------------------------------------
# With q(v_t) fixed in whitened coordinates and the noise fixed by (n_f, seed), fit_q_softmax_'s bound
#     value = sum_n w_n [mu_{y_n, n} - mean_f logsumexp(mu_n + sqrt(var_n) o eps_nf)] - sum_c KL(q(v_t, c) || N(0, I))
# is a deterministic function of the inducing points and theta through alpha, Q and k_n.  Its gradient is the EXACT derivative of
# that n_f-sample estimate (s the upstream seed):
#     gm_cn = s w_n ([y_n = c] - mean_f p_c),   gv_cn = -s w_n / (2 sqrt(var_cn)) mean_f (p_c eps_c)  (var_cn > 0; else exactly 0)
# -- the pathwise derivative for var, NOT the Price estimate -1/2 E p (1 - p) behind the E-step's lam2: the M-step ascends a
# deterministic function whose values the undo rule compares, and only the exact derivative can be held against autograd.  (The
# sampled objective has an unbounded slope as var -> 0+; nothing guards against it, and at var = 0 the derivative is 0 by the
# convention of ell_torch.)  Everything behind (gm, gv) is the site bound's algebra with the seeds given: ops.site_transport_bwd
# and gQ = -gram_moments(w = gv u).Phi.  Four launches-with-reduce forward and back: ops.site_marginals, ops.softmax_sites |
# ops.softmax_site_grads, ops.site_transport_bwd, ops.gram_moments.
# CAVEAT: the E-step's Bonnet / Price sites are not the stationarity condition of the SAMPLED bound, so at the E-step's q the
# partial gradient for (z, theta) is the gradient of the re-converged bound only up to the Monte-Carlo error of the sites: the
# envelope argument of fit_sites_ is approximate here, and it is the undo rule that guarantees a non-decreasing trace.
def check_softmax_differentiable(gp, who):
    """check_softmax_supported, and exactly RBFKernel or MaternKernel: a DeepRBFKernel is refused for check_differentiable's
    reason.  Needs no device."""
    _SoftmaxProblem.check(gp, who, differentiable=True)


def softmax_value_torch(mu, var, y, w, eps):
    """sum_n w_n [mu_{y_n, n} - mean_f logsumexp(mu_n + sqrt(var_n) eps_nf)] () float64 in fp32 elementwise torch (summed in fp64),
    differentiable in mu and var (C, B); eps (F, C, B).  sqrt has no derivative at a variance of 0: that of 1, times 0 (ell_torch's
    convention).  Any device."""
    pos = var > 0
    sd = torch.where(pos, torch.where(pos, var, torch.ones_like(var)).sqrt(), torch.zeros_like(var))
    lse = torch.logsumexp(mu + sd * eps, -2).mean(0)
    hot = (y.unsqueeze(0) == torch.arange(mu.size(0), device=y.device).unsqueeze(1)).to(mu.dtype)
    ell = ((mu * hot).sum(0) - lse).double()
    if w is None:
        return ell.sum()
    return torch.where(w != 0, w.double() * ell, torch.zeros_like(ell)).sum()


def _softmax_tile_value(leaves, Xt, yt, wt, eps_t, nu2):
    """sum_n w_n ell_n () float64 of one tile of points from the differentiable per-op nodes (the gram op, ops.matmul) and
    softmax_value_torch on the tile's noise eps_t (F, C, B).  leaves: theta, Z, alpha, Q."""
    theta, Z, alpha, Q = leaves
    mu, var = _tile_marginals(_gram_tile(theta.view(1, -1), Z, Xt, nu2), alpha, 0.5 * (Q + Q.mT), (2.0 * theta[-1]).exp())
    return softmax_value_torch(mu, var, yt, wt, eps_t)


def composed_softmax_site_bound(theta, Z, X, alpha, Q, y, w, n_f, seed=0, eps=None, nu2=0, tile=COMPOSED_TILE):
    """ops.softmax_site_bound_diff from the per-op kernels (arguments alike, any Mt; value (1,) float64) on an explicit noise
    tensor (eps, or ops.softmax_site_noise(seed, n_f, C, N): n_f C N floats), sliced per tile: the route above ops.SITE_MAX_MT
    inducing points and the on-device yardstick of the fused backward."""
    ops.require_device(theta, Z, X, alpha, Q, y, w, eps)
    ops.refuse_grad('composed_softmax_site_bound', ops.SOFTMAX_BOUND_GRADS, X=X, y=y, w=w)
    if eps is None:
        eps = ops.softmax_site_noise(seed, n_f, Z.size(0), X.size(0), device=X.device)
    assert tuple(eps.shape) == (int(n_f), Z.size(0), X.size(0)), (eps.shape, n_f, Z.shape, X.shape)
    return _ComposedBound.apply(_softmax_tile_value, lambda n0, n1: (eps[:, :, n0:n1], int(nu2)), 1, int(tile), X, y, w, theta, Z, alpha, Q)


def softmax_site_bound(gp, x, y, weights=None, q=None, route=None, n_f=32, seed=0):
    """fit_q_softmax_'s bound of the data x (N, D), y (N,) int64 -- the n_f-sample estimate of the data term with the noise of
    `seed`, minus sum_c KL(q(v_t, c) || N(0, I)) -- as a (1,) float64 ON THE AUTOGRAD GRAPH of gp.z and gp.kernel.log_mean.
    q = (a_t (C, M), H_t (C, M, M) lower) is q(u_t) in whitened coordinates and a CONSTANT; None: whitened_q(gp), with which the
    value is fit_q_softmax_(n_iters=0, n_f, seed).bound[0].  The frozen tasks are constants whose whitened moments are
    differentiated through the whitening, as in site_bound.  The gradient is the exact derivative of the sampled value (the
    comment above).  route 'fused' (up to ops.SITE_MAX_MT inducing points over all tasks; K(z, x) is never stored) or 'composed'
    (above it or on request: per-op kernels, a tile of N at a time, on an explicit noise tensor of n_f C N floats).
    MulticlassSoftmax, ep_var_mean=True, exactly RBFKernel or MaternKernel, at most ops.SOFTMAX_SITE_MAX_C classes.  The
    hyper-prior (kl_hypers) is NOT part of the bound."""
    return _bound(_SoftmaxProblem, gp, x, y, weights, q, route, 'softmax_site_bound', n_f=n_f, seed=seed)


def fit_softmax_sites_(gp, x, y, n_rounds=5, m_steps=20, lr=1e-2, params=None, newton_iters=20, damping=1.0, tol=1e-6, weights=None,
                       route=None, start='current', n_f=32, seed=0):
    """fit_sites_ for MulticlassSoftmax: variational EM on the softmax site bound, full batch and in place.  E-step
    fit_q_softmax_(n_iters=newton_iters, damping, tol, n_f, seed); M-step m_steps Yogi steps on -softmax_site_bound with the same
    (n_f, seed) -- one deterministic function for the whole fit -- over the subset `params` of {'z': gp.z, 'kernel':
    gp.kernel.log_mean} (None: both; the softmax has no parameter, 'lik' is a ValueError), with q held at the E-step's whitened
    (a_t, H_t), then set_whitened_q_.  The undo rule and `stopped` are fit_sites_': the trace never falls.  The E-step's sites
    are Bonnet / Price estimates, not the stationarity condition of the sampled bound, so the M-step's partial gradient is the
    re-converged bound's only approximately; the undo rule is what guarantees monotonicity.  The hyper-prior is NOT in the
    objective.  -> EMFit(bound (n_rounds + 1, 1) float64 on the host, n_rounds, n_newton, stopped)."""
    return _fit_em(_SoftmaxProblem, gp, x, y, n_rounds, m_steps, lr, params, newton_iters, damping, tol, weights, route, start,
                   n_f=n_f, seed=seed)
