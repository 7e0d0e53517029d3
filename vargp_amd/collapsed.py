"""The optimal q(u) of a Gaussian-likelihood model in closed form (Titsias' collapsed bound, SGPR) -- not in the reference, whose
q(u) is only ever moved by gradient steps.  `fit_q_` (VARGP.fit_q_, create_reg(q_init='optimal')) writes it into u_mean and
u_tril_vec and returns the bound's value at the optimum; for a Gaussian likelihood this is one natural-gradient step of length 1.
`collapsed_bound` is the same value on the autograd graph of z, kernel.log_mean and obs_log_var, and `fit_collapsed_` climbs it
(SGPR: no q(u) parameter; VARGP.collapsed_bound, VARGP.fit_collapsed_, create_reg(q_init='collapsed')).

Everything happens at ONE hyper vector, theta = kernel.log_mean, in the whitened coordinates of whitened.py's docstring (K' = L L^T,
T = L^-1, v = T u, q(v) = N(a, H H^T) with the frozen tasks' blocks a_i, H_i; A, tc, the reversed Cholesky and the writer are
defined there).  The data enter through two weighted moments of the cross-kernel, Phi = sum_n w_n k_n k_n^T and
c = sum_n w_n y_n k_n, k_n = k(z_<=t, x_n) (ops.gram_moments, csrc/moments.hip: K(z, X) is never stored), and sw = sum_n w_n,
syy = sum_n w_n y_n^2.  With A = T Phi T^T, tc = T c, beta = temper / sigma^2 per output, `<` the earlier tasks and `t` the new
block:

    b_t     = tc_t - A_{t,<} a_<
    Sigma_t = (I + beta A_tt)^-1           a_t = beta Sigma_t b_t
    u_mean  = L_tt a_t                     u_tril = chol(L_tt Sigma_t L_tt^T)
    bound   = -1/2 sw log(2 pi / beta)
              - 1/2 beta [syy - 2 a_<^T tc_< + a_<^T A_<< a_< + gamma^2 sw - tr A + sum_{i<t} tr(H_i^T A_ii H_i)]
              + 1/2 beta^2 b_t^T Sigma_t b_t - 1/2 logdet(I + beta A_tt)

`bound` = E_q log N(y | f, 1 / beta) - KL(q(v_t) || N(0, I)) at its maximum over (a_t, H_t): the standard variational bound of the
new task's data (tests/test_collapsed.py restates all of this in fp64, checks that the bound's gradient vanishes there and that the
closed form equals the evaluated bound).  Sigma_t has its eigenvalues in (0, 1] whatever the conditioning of K'.  u_tril comes
without a second factorisation: I + beta A_tt = U U^T with U upper triangular (whitened.reversed_chol), so Sigma_t = G G^T with
G = U^-T lower triangular and u_tril = L_tt G.

CAVEAT: GaussianLikelihood.loss is the reference's -log N(y | mu, var + sigma^2) (its mean over outputs), not -E_q log p(y | f).
fit_q_ maximises the standard bound above, so the q(u) it writes is NOT exactly the minimiser of kl_u + nll as VARGP.loss
reports them (the two agree as the predictive variance becomes small against sigma^2); the loss is left as it is."""
import math
from collections import namedtuple

import torch

from . import ops
from .likelihoods import GaussianLikelihood
from .optim import ascend_, choose_params
from .whitened import Frame, check_model, mv, reversed_chol, rows, whiten_moments, write_q_
from .whitened import inv_softplus  # noqa: F401  (public here too: the inverse of the diagonal map of u_tril_vec that fit_q_ writes)

CollapsedFit = namedtuple('CollapsedFit', 'bound n_chunks')
CollapsedFit.__doc__ = """bound (C,) float64: per output, the variational bound of the fitted data at the optimal q(u) (nats);
n_chunks: the number of chunks the moment kernel cut the N points into (ops.gram_moments_chunks)."""


def _check_likelihood(lik, who):
    if not isinstance(lik, GaussianLikelihood):
        raise ValueError(f'{who}: the closed-form q(u) exists for GaussianLikelihood only (create_reg(likelihood="gaussian")), '
                         f'got {type(lik).__name__}')


def check_supported(gp, who='fit_q_'):
    """ValueError unless the closed form applies to the model: GaussianLikelihood, ep_var_mean=True, an RBF / Matern / deep-RBF
    kernel.  Needs no device."""
    check_model(gp, who, _check_likelihood)


def _whitened_bound(gp, x, y, weights, temper):
    """The module docstring's formulas, once, for fit_q_ and collapsed_bound alike: every step is a differentiable op (or fp64
    elementwise torch), so under no_grad this is the plain computation and otherwise the bound sits on the autograd graph of gp.z,
    kernel.log_mean and obs_log_var.  -> (bound (C,) float64, n_chunks, what fit_q_ needs for q(u_t): beta, L_tt, G, G64, gb)."""
    fr = Frame(gp)
    C, M, N, n_lt = fr.C, fr.M, x.size(0), fr.n_lt
    wt = None if weights is None else rows(weights, C, N)
    zf, xf = fr.operands(x)

    # the only pass over the data (and, in the backward, the only other one); BEFORE the factorisation (whitened.py: ORDER)
    Phi, c, sums = ops.gram_moments_diff(fr.theta, zf, xf, wt, rows(y, C, N), fr.nu2)
    n_chunks = ops.gram_moments_chunks(C, fr.Mt, N, zf.size(-1))

    A, tc = whiten_moments(fr.T, Phi, c)
    sw, syy = sums[:, 0].double(), sums[:, 1].double()
    beta = float(temper) * (-gp.likelihood.obs_log_var.double()).exp()               # (C,)
    g2 = (2.0 * fr.theta[-1].double()).exp()

    # the frozen tasks: a_< and sum_i tr(H_i^T A_ii H_i)
    a_lt, H_lt = fr.frozen
    trHAH, o = torch.zeros(C, dtype=torch.float64, device=x.device), 0
    for H in H_lt:
        n, H = H.size(-1), H.double()
        A_ii = A[:, o:o + n, o:o + n]
        trHAH = trHAH + ((A_ii.unsqueeze(-1) * H.unsqueeze(-3)).sum(-2) * H).sum((-2, -1))
        o += n
    A_ll, A_tl, A_tt = A[:, :n_lt, :n_lt], A[:, n_lt:, :n_lt], A[:, n_lt:, n_lt:]
    b_t = tc[:, n_lt:] - mv(A_tl, a_lt)

    # Sigma_t = (I + beta A_tt)^-1 = G G^T
    Lr, G = reversed_chol(torch.eye(M, dtype=torch.float64, device=x.device) + beta.view(C, 1, 1) * A_tt)
    G64 = G.double().tril()
    gb = mv(G64.mT, b_t)
    quad = gb.square().sum(-1)                                                        # b_t^T Sigma_t b_t
    logdet = 2.0 * Lr.diagonal(dim1=-2, dim2=-1).double().log().sum(-1)

    fixed = syy - 2.0 * (a_lt * tc[:, :n_lt]).sum(-1) + (a_lt * mv(A_ll, a_lt)).sum(-1) + g2 * sw \
        - A.diagonal(dim1=-2, dim2=-1).sum(-1) + trHAH
    bound = -0.5 * sw * (2.0 * math.pi / beta).log() - 0.5 * beta * fixed + 0.5 * beta.square() * quad - 0.5 * logdet
    return bound, n_chunks, (beta, fr.L_tt, G, G64, gb)


def fit_q_(gp, x, y, weights=None, temper=1.0):
    """Set q(u_t) of the VARGP model `gp` to its optimum for the data x (N, D), y (N,) or (C, N) (as loss() takes it), in place and
    under no_grad; weights None, (N,) or (C, N), >= 0: per-point weights of the log-likelihood; temper: a factor on all of them
    (beta = temper / sigma^2).  First-task models and models with prev_params alike; hyper-parameters, inducing points and
    obs_log_var are read, not changed.  -> CollapsedFit(bound (C,) float64, n_chunks).  See the module docstring for the formulas
    and for how the bound relates to VARGP.loss."""
    check_supported(gp)
    ops.require_device(gp.z, x, y, weights)
    with torch.no_grad():
        bound, n_chunks, (beta, L_tt, G, G64, gb) = _whitened_bound(gp, x, y, weights, temper)
        write_q_(gp, L_tt, beta.unsqueeze(-1) * mv(G64, gb), G)
    return CollapsedFit(bound, n_chunks)


def check_differentiable(gp, who):
    """check_supported, and exactly RBFKernel or MaternKernel: the bound's gradient for a DeepRBFKernel needs the gradient of the
    moments for X (the feature map), which ops.gram_moments_diff does not produce."""
    check_model(gp, who, _check_likelihood, deep='the feature map needs the gradient of the moments for their inputs X, which '
                                                 'the fused backward does not produce); fit_q_ supports it')


def collapsed_bound(gp, x, y, weights=None, temper=1.0):
    """Titsias' collapsed bound of the data x (N, D), y (N,) or (C, N) -- the value fit_q_ returns, the variational bound at the
    optimal q(u_t) -- as a (C,) float64 tensor ON THE AUTOGRAD GRAPH of gp.z, gp.kernel.log_mean and gp.likelihood.obs_log_var
    (the module docstring's formulas; the frozen tasks' inducing points and q(u) are constants).  q(u_t) itself is neither read
    nor written.  x, y and weights get no gradient.  One fused pass over the data forward and one backward
    (ops.gram_moments_diff): K(z, x) is never stored in either.  GaussianLikelihood, ep_var_mean=True, exactly RBFKernel or
    MaternKernel; a DeepRBFKernel is refused (ValueError).  The hyper-prior (kl_hypers) is NOT part of the bound."""
    check_differentiable(gp, 'collapsed_bound')
    ops.require_device(gp.z, x, y, weights)
    return _whitened_bound(gp, x, y, weights, temper)[0]


def fit_collapsed_(gp, x, y, n_steps=200, lr=1e-2, weights=None, temper=1.0, params=('z', 'kernel', 'noise')):
    """Full-batch ascent of sum_c collapsed_bound over the chosen subset of {'z': gp.z, 'kernel': gp.kernel.log_mean, 'noise':
    gp.likelihood.obs_log_var} with the project's Yogi (optim.py), n_steps deterministic steps without any q(u) parameter, then
    fit_q_ once at the parameters reached.  The objective is the bound alone: the hyper-prior (kl_hypers) is NOT in it, so this
    is maximum likelihood (type II) for the hyper-parameters, not the MAP / variational treatment of VARGP.loss.
    -> the bound per step, float64 (n_steps + 1, C) on the host: row k is the bound BEFORE step k + 1, the last row the bound
    fit_q_ reports at the final parameters.  One device synchronisation, at the end."""
    check_differentiable(gp, 'fit_collapsed_')
    chosen = choose_params('fit_collapsed_', dict(z=gp.z, kernel=gp.kernel.log_mean, noise=gp.likelihood.obs_log_var), params)
    n_steps = int(n_steps)
    if n_steps < 0:
        raise ValueError(f'fit_collapsed_: n_steps must be >= 0, got {n_steps}')
    ops.require_device(gp.z, x, y, weights)
    trace = ascend_(lambda: collapsed_bound(gp, x, y, weights=weights, temper=temper), chosen, n_steps, lr)
    trace.append(fit_q_(gp, x, y, weights=weights, temper=temper).bound)
    return torch.stack(trace).cpu()
