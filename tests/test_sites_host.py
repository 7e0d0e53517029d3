"""The natural-gradient q(u) fit for the non-Gaussian likelihoods (vargp_amd/sites.py, VARGP.fit_q_newton_), the part that needs
no GPU: a dense fp64 restatement in plain torch of one site pass (csrc/sites.hip) and of the whole iteration -- what
tests/test_hip_sites.py measures the device against -- with the 20-node rule of numpy.polynomial.hermite.hermgauss(20), checked
against itself: with the sites of a Gaussian likelihood one full step is the closed form restated in tests/test_collapsed.py, and
for Bernoulli and Poisson data the accepted trace never falls and the gradient of the EVALUATED bound (autograd through the
quadrature) vanishes at the q the loop stops at.  Then the C-ABI entry's exports and argument checks and the ValueErrors of
fit_q_newton_ and the factories."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_collapsed import _Data, make_problem, ref_fit, ref_kernel, ref_whiten

F64 = torch.float64
_X, _W = np.polynomial.hermite.hermgauss(20)
GH_X, GH_W = torch.tensor(_X, dtype=F64), torch.tensor(_W / math.sqrt(math.pi), dtype=F64)
KINDS = ('probit', 'logit', 'poisson', 'studentt')          # ... and 'gauss' (par: beta (G,)), for the closed-form check only


# -- the restatement ----------------------------------------------------------------------------------------------------------------
def _logp(kind, par, f, y):
    """log p(y | f) at the nodes f (.., 20); y (.., 1).  par: dict(log_scale (G,), df) for 'studentt', dict(beta (G,)) for 'gauss'."""
    if kind == 'probit':
        return torch.special.log_ndtr((2.0 * y - 1.0) * f)
    if kind == 'logit':
        return torch.nn.functional.logsigmoid((2.0 * y - 1.0) * f)
    if kind == 'poisson':
        return y * f - f.exp() - torch.lgamma(y + 1.0)
    if kind == 'studentt':
        ls, df = par['log_scale'].to(F64).view(-1, 1, 1), float(par['df'])
        k = math.lgamma(0.5 * (df + 1.0)) - math.lgamma(0.5 * df) - 0.5 * math.log(df * math.pi) - ls
        return k - 0.5 * (df + 1.0) * torch.log1p((y - f).square() * (-2.0 * ls).exp() / df)
    beta = par['beta'].to(F64).view(-1, 1, 1)
    return -0.5 * (2.0 * math.pi / beta).log() - 0.5 * beta * (y - f).square()


def ref_ell(kind, par, mu, var, y):
    """E_{f ~ N(mu, var)} log p(y | f), (G, N) fp64, differentiable in mu and var > 0: the 20-node rule; Poisson and Gauss in
    their closed forms (for which the rule is not what the kernels evaluate)."""
    if kind == 'poisson':
        return y * mu - (mu + 0.5 * var).exp() - torch.lgamma(y + 1.0)
    if kind == 'gauss':
        beta = par['beta'].to(F64).view(-1, 1)
        return -0.5 * (2.0 * math.pi / beta).log() - 0.5 * beta * ((y - mu).square() + var)
    f = mu.unsqueeze(-1) + (2.0 * var).sqrt().unsqueeze(-1) * GH_X
    return (_logp(kind, par, f, y.unsqueeze(-1)) * GH_W).sum(-1)


def ref_ell_derivs(kind, par, mu, var, y):
    """-> ell, d ell / d mu, d ell / d var as csrc/lik.h defines them: with g = d log p / d f at the nodes,
    dmu = sum_k w_k g_k and dvar = sum_k w_k x_k g_k / sqrt(2 var), which is DEFINED as 0 at var = 0 (every node is then the same
    point and the sum cancels exactly)."""
    mu, var, y = mu.detach(), var.detach(), y.detach()
    ell = ref_ell(kind, par, mu, var, y)
    if kind == 'poisson':
        e = (mu + 0.5 * var).exp()
        return ell, y - e, -0.5 * e
    if kind == 'gauss':
        beta = par['beta'].to(F64).view(-1, 1)
        return ell, beta * (y - mu), (-0.5 * beta).expand_as(mu)
    sd = (2.0 * var).sqrt().unsqueeze(-1)
    f = (mu.unsqueeze(-1) + sd * GH_X).requires_grad_(True)
    g, = torch.autograd.grad(_logp(kind, par, f, y.unsqueeze(-1)).sum(), f)
    # (at var = 0 the twenty g are one value and the signed sum is rounding noise, not the exact 0 of the kernels' +-x_k pairs)
    dvar = torch.where(var > 0, (g * GH_W * GH_X).sum(-1) / sd.squeeze(-1).clamp_min(1e-300), torch.zeros_like(var))
    return ell, (g * GH_W).sum(-1), dvar


def ref_sites(kind, par, theta, Z, X, alpha, Q, y, w, nu2):
    """One site pass, dense fp64 (the formulas of csrc/sites.hip).  Z (G, Mt, D), X (N, D), alpha (G, Mt), Q (G, Mt, Mt), y (G, N)
    or (N,), w (G, N) or None -> dict(lam2 (G, N), c (G, Mt), sums (G, 4), Phi (G, Mt, Mt), mu, var)."""
    theta, Z, X, alpha, Q, y = (t.to(F64) for t in (theta, Z, X, alpha, Q, y))
    K = ref_kernel(Z, X.unsqueeze(0), theta, nu2)                                   # (G, Mt, N)
    y = y.expand(K.shape[0], -1)
    w = torch.ones_like(y) if w is None else w.to(F64)
    mu = (alpha.unsqueeze(-1) * K).sum(-2)
    var = ((2.0 * theta[-1]).exp() - (K * (Q @ K)).sum(-2)).clamp_min(0.0)
    ell, dmu, dvar = ref_ell_derivs(kind, par, mu, var, y)
    on, zero = w != 0, torch.zeros_like(mu)
    lam2 = torch.where(on, w * (-2.0 * dvar).clamp_min(0.0), zero)
    lam1 = torch.where(on, w * dmu + lam2 * mu, zero)
    sums = torch.stack([torch.where(on, w * ell, zero).sum(-1), lam2.sum(-1), (on & (dvar > 0)).to(F64).sum(-1), w.sum(-1)], -1)
    return dict(lam2=lam2, c=(K * lam1.unsqueeze(-2)).sum(-1), sums=sums, Phi=(K * lam2.unsqueeze(-2)) @ K.mT, mu=mu, var=var)


def _mv(B, v):
    return (B @ v.unsqueeze(-1)).squeeze(-1)


def _kl(a_t, Sigma):
    M = a_t.shape[-1]
    return 0.5 * (a_t.square().sum(-1) + Sigma.diagonal(dim1=-2, dim2=-1).sum(-1) - M - torch.linalg.slogdet(Sigma)[1])


def ref_newton(kind, par, theta, z_all, prev, x, y, w, nu2, u_mean0, u_tril0, n_iters=20, damping=1.0, tol=1e-6, max_halvings=8):
    """sites.fit_q_newton_ restated dense in fp64.  z_all (C, Mt, D): all tasks' inducing points; prev: the frozen tasks as
    ref_whiten takes them; u_mean0 (C, M, 1), u_tril0 (C, M, M): the starting q(u_t).  -> dict(u_mean (C, M), S_u (C, M, M) =
    L_u L_u^T, a_t, Sigma_t, trace (n + 1, C), n_iters, n_rejected, n_clamped)."""
    L, T, a_lt, H = ref_whiten(theta, z_all, prev, nu2)
    C, Mt = z_all.shape[:2]
    M = u_mean0.shape[-2]
    n_lt = Mt - M
    T_tt, L_tt = T[:, n_lt:, n_lt:], L[:, n_lt:, n_lt:]
    eye = torch.eye(M, dtype=F64)
    y64 = y.to(F64)

    def sites_at(a_t, Sigma):
        a = torch.cat([a_lt, a_t], -1)
        HH = torch.stack([torch.block_diag(*[(Hi[c] @ Hi[c].mT) for Hi in H], Sigma[c]) for c in range(C)])
        Q = T.mT @ (torch.eye(Mt, dtype=F64) - HH) @ T
        s = ref_sites(kind, par, theta, z_all, x, _mv(T.mT, a), 0.5 * (Q + Q.mT), y64, w, nu2)
        A = T @ s['Phi'] @ T.mT
        tc = _mv(T, s['c'])
        return (s['sums'][:, 0] - _kl(a_t, Sigma), eye + A[:, n_lt:, n_lt:], tc[:, n_lt:] - _mv(A[:, n_lt:, :n_lt], a_lt),
                s['sums'][:, 2])

    a_t = _mv(T_tt, u_mean0.to(F64).squeeze(-1))
    H_t = T_tt @ u_tril0.to(F64)
    Sigma = H_t @ H_t.mT
    P = torch.linalg.inv(Sigma)
    P = 0.5 * (P + P.mT)
    h = _mv(P, a_t)
    bound, P_new, h_new, clamped = sites_at(a_t, Sigma)
    trace, n_rejected = [bound], 0
    while len(trace) - 1 < n_iters:
        rho, accepted = damping, None
        for _ in range(max_halvings + 1):
            P_c, h_c = (1.0 - rho) * P + rho * P_new, (1.0 - rho) * h + rho * h_new
            S_c = torch.linalg.inv(P_c)
            S_c = 0.5 * (S_c + S_c.mT)
            a_c = _mv(S_c, h_c)
            bound_c, P_next, h_next, clamped_c = sites_at(a_c, S_c)
            if bool(torch.isfinite(bound_c).all()) and bool((bound_c >= trace[-1]).all()):
                accepted = (P_c, h_c, a_c, S_c, P_next, h_next, clamped_c)
                break
            n_rejected += 1
            rho *= 0.5
        if accepted is None:
            break
        P, h, a_t, Sigma, P_new, h_new, clamped = accepted
        trace.append(bound_c)
        if (trace[-1].sum() - trace[-2].sum()).item() < tol * abs(trace[-1].sum().item()):
            break
    S_u = L_tt @ Sigma @ L_tt.mT
    return dict(u_mean=_mv(L_tt, a_t), S_u=0.5 * (S_u + S_u.mT), a_t=a_t, Sigma_t=Sigma, trace=torch.stack(trace),
                n_iters=len(trace) - 1, n_rejected=n_rejected, n_clamped=int(clamped.sum().item()))


def ref_site_bound(kind, par, theta, z_all, prev, x, y, w, nu2, a_t, H_t):
    """The bound for ANY q(v_t) = N(a_t, H_t H_t^T), fp64, summed point by point from the dense K(z, x) and differentiable in
    a_t and H_t: E_q log p(y_n | f_n) by ref_ell at mean p_n^T a and variance |H^T p_n|^2 + gamma^2 - |p_n|^2, p_n = T k_n."""
    L, T, a_lt, H = ref_whiten(theta, z_all, prev, nu2)
    M = a_t.shape[-1]
    y = y.to(F64)
    P = T @ ref_kernel(z_all.to(F64), x.to(F64).unsqueeze(0), theta.to(F64), nu2)
    y = y.expand(P.shape[0], -1)
    w = torch.ones_like(y) if w is None else w.to(F64)
    a = torch.cat([a_lt, a_t], -1)
    Hb = torch.stack([torch.block_diag(*[Hi[c] for Hi in H], H_t[c]) for c in range(a.shape[0])])
    mean = (P * a.unsqueeze(-1)).sum(-2)
    var = ((Hb.mT @ P) ** 2).sum(-2) + (2.0 * theta[-1].to(F64)).exp() - (P * P).sum(-2)
    return (w * ref_ell(kind, par, mean, var, y)).sum(-1) - _kl(a_t, H_t @ H_t.mT)


def default_q(C, M, seed):
    """The model's default start in the restatement's terms: u_mean ~ N(0, 0.25), u_tril = softplus(1) I."""
    g = torch.Generator().manual_seed(seed)
    u_mean = 0.5 * torch.randn(C, M, 1, generator=g)
    return u_mean, math.log1p(math.e) * torch.eye(M).expand(C, M, M).contiguous()


def make_targets(kind, pr, seed):
    """Targets of `kind` for the inputs of a test_collapsed.make_problem: a smooth latent per output, then labels / counts /
    heavy-tailed noise.  -> y (C, N) float32"""
    g = torch.Generator().manual_seed(seed)
    f = pr['y']                                                                     # the smooth function + small noise
    if kind in ('probit', 'logit'):
        return (torch.rand(f.shape, generator=g) < torch.sigmoid(3.0 * f)).float()
    if kind == 'poisson':
        return torch.poisson((0.8 * f + 0.5).exp(), generator=g)
    return f + 0.05 * torch.distributions.StudentT(4.0).sample(f.shape)


# -- the restatement against itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [0, 1])
def test_gaussian_sites_give_the_closed_form_in_one_full_step(t):
    """lam2 = beta, lam1 = beta y: one rho = 1 step from the default q(u) is test_collapsed.ref_fit's optimum (temper = 1)."""
    pr = make_problem(2, 5, t, 3, 40, seed=20 + t, weights=True)
    fit = ref_fit(pr['theta'], pr['z_all'], pr['prev'], pr['x'], pr['y'], pr['w'], pr['obs_log_var'], 0)
    u_mean0, u_tril0 = default_q(2, 5, 1)
    par = dict(beta=(-pr['obs_log_var']).exp())
    got = ref_newton('gauss', par, pr['theta'], pr['z_all'], pr['prev'], pr['x'], pr['y'], pr['w'], 0, u_mean0, u_tril0, n_iters=1)
    assert got['n_iters'] == 1 and got['n_rejected'] == 0
    # the step forms lam1 = beta (y - mu_0) + beta mu_0 at the STARTING q, whose mean mu_0 is large (|T| up to jitter^-1/2 = 100
    # twice over: |mu_0| ~ 1e3..1e4, beta ~ 20): the cancellation costs eps64 * beta |mu_0| ~ 1e-11 per point, times N |T| ~ 4e3
    # on the way to a_t -- 1e-7, not the 1e-9 of the closed form's own check
    tol = 1e-7
    assert torch.allclose(got['a_t'], fit['a_t'], rtol=0, atol=tol) and torch.allclose(got['Sigma_t'], fit['Sigma_t'], rtol=0, atol=tol)
    assert torch.allclose(got['u_mean'], fit['u_mean'], rtol=0, atol=tol)
    assert torch.allclose(got['S_u'], fit['u_tril'] @ fit['u_tril'].mT, rtol=0, atol=tol)
    # the bound after the step is the collapsed bound
    assert torch.allclose(got['trace'][-1], fit['bound'], rtol=tol, atol=0)


# iterations the restatement takes to tol = 1e-10 from the default q(u) on the problems below (no rejected step), recorded from
# this test's own output: (kind, t) -> accepted steps
RECORDED_ITERS = {('probit', 0): 6, ('probit', 1): 5, ('logit', 0): 5, ('poisson', 0): 8, ('poisson', 1): 9}


@pytest.mark.parametrize('kind,t', sorted(RECORDED_ITERS))
def test_trace_rises_and_the_gradient_vanishes_at_convergence(kind, t):
    """M = 5, D = 3, N = 60, two outputs, weights: the accepted trace is non-decreasing without a rejected step, the loop stops
    within 20 iterations, and autograd's gradient of the evaluated bound for (a_t, chol Sigma_t) at the end is below 1e-5 of its
    norm at the start.  (The loop stops once a step gains less than tol |bound| ~ 1e-10 * 300 nats; a Newton step gains about
    g^T P^-1 g / 2, so the gradient BEFORE that step is about sqrt(2 * 3e-8 * |P|) with |P| up to ~1e3, i.e. below 1e-2, and the
    last step contracts it quadratically: 1e-5 of a starting norm of ~1e2 is a loose bound.  Measured: poisson t = 0, 8e-7.)"""
    pr = make_problem(2, 5, t, 3, 60, seed=30 + t, weights=True)
    y = make_targets(kind, pr, 5)
    u_mean0, u_tril0 = default_q(2, 5, 2)
    args = (kind, {}, pr['theta'], pr['z_all'], pr['prev'], pr['x'], y, pr['w'], 0)
    got = ref_newton(*args, u_mean0, u_tril0, n_iters=20, tol=1e-10)
    tr = got['trace']
    print(f'{kind} t={t}: {got["n_iters"]} iterations, rejected {got["n_rejected"]}, trace {tr.sum(-1).tolist()}')
    assert got['n_rejected'] == 0 and got['n_iters'] < 20 and got['n_clamped'] == 0
    assert got['n_iters'] == RECORDED_ITERS[(kind, t)]
    assert bool((tr[1:] >= tr[:-1]).all()) and bool((tr[-1] > tr[0]).all())

    def grad_norm(a_t, Sigma):
        a = a_t.clone().requires_grad_(True)
        Hr = torch.linalg.cholesky(Sigma).clone().requires_grad_(True)
        val = ref_site_bound(*args, a, Hr.tril())
        ga, gH = torch.autograd.grad(val.sum(), (a, Hr))
        return math.sqrt(ga.square().sum().item() + gH.tril().square().sum().item()), val.detach()

    _, T, _, _ = ref_whiten(pr['theta'], pr['z_all'], pr['prev'], 0)
    T_tt = T[:, -5:, -5:]
    H0 = T_tt @ u_tril0.double()
    g0, v0 = grad_norm((T_tt @ u_mean0.double()).squeeze(-1), H0 @ H0.mT)
    g1, v1 = grad_norm(got['a_t'], got['Sigma_t'])
    print(f'  |grad| start {g0:.3e} end {g1:.3e}')
    assert g1 < 1e-5 * g0
    # the evaluated bound is the trace's: first and last row
    assert torch.allclose(v0, tr[0], rtol=1e-10, atol=1e-10) and torch.allclose(v1, tr[-1], rtol=1e-10, atol=1e-10)


def test_studentt_outlier_is_clamped_and_the_loop_still_climbs():
    """A gross outlier makes d ell / d var positive at the start: the clamp is counted, and the accepted trace still rises."""
    pr = make_problem(1, 5, 0, 2, 40, seed=41)
    y = make_targets('studentt', pr, 6)
    y[0, 3] += 25.0
    par = dict(log_scale=torch.tensor([-1.5]), df=4.0)
    u_mean0, u_tril0 = default_q(1, 5, 3)
    Z, th = pr['z_all'], pr['theta']
    L, T, _, _ = ref_whiten(th, Z, [], 0)
    a0 = (T @ u_mean0.double()).squeeze(-1)
    H0 = T @ u_tril0.double()
    Q = T.mT @ (torch.eye(5, dtype=F64) - H0 @ H0.mT) @ T
    s = ref_sites('studentt', par, th, Z, pr['x'], _mv(T.mT, a0), Q, y, None, 0)
    assert s['sums'][0, 2].item() >= 1 and s['lam2'][0, 3].item() == 0.0
    got = ref_newton('studentt', par, th, Z, [], pr['x'], y, None, 0, u_mean0, u_tril0)
    assert bool((got['trace'][1:] >= got['trace'][:-1]).all()) and got['n_iters'] >= 1


def test_zero_variance_and_zero_weight_in_the_restatement():
    """var clamped to 0 (one inducing point with the point on it and Q > gamma^-2): dvar is 0 by definition for the quadrature kinds; a
    zero-weight point adds nothing whatever its target."""
    th = torch.tensor([0.0, 0.0, math.log(0.9)])
    Z = torch.tensor([[[0.3, -0.2]]])
    X = torch.tensor([[0.3, -0.2], [1.0, 1.0]])
    Q = torch.tensor([[[3.0]]])
    s = ref_sites('probit', {}, th, Z, X, torch.tensor([[0.5]]), Q, torch.tensor([[1.0, 0.0]]), None, 0)
    assert s['var'][0, 0].item() == 0.0 and s['lam2'][0, 0].item() == 0.0 and s['var'][0, 1].item() > 0.0
    w = torch.tensor([[1.0, 0.0]])
    a = ref_sites('poisson', {}, th, Z, X, torch.tensor([[0.5]]), Q, torch.tensor([[1.0, 3.0]]), w, 0)
    b = ref_sites('poisson', {}, th, Z, X, torch.tensor([[0.5]]), Q, torch.tensor([[1.0, 1e6]]), w, 0)
    assert torch.equal(a['c'], b['c']) and torch.equal(a['sums'], b['sums']) and a['lam2'][0, 1].item() == 0.0


# -- the C ABI ----------------------------------------------------------------------------------------------------------------------
SITE_SYMBOLS = ('vargp_site_moments', 'vargp_site_moments_workspace_bytes', 'vargp_site_moments_chunks')


def test_site_symbols_are_exported_and_declared():
    from vargp_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'vargp_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in SITE_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(handle, name) and hasattr(_lib.lib(), name)
        assert re.search(r'\b%s\s*\(' % name, text), f'{name} is not declared in include/vargp_hip.h'


def test_site_workspace_and_chunks():
    """Per-chunk partials only; the chunk count is a function of the shapes: at least 256 columns per chunk, at most 1024."""
    from vargp_amd import ops
    from vargp_amd._lib import lib
    ws, chunks = lib().vargp_site_moments_workspace_bytes, lib().vargp_site_moments_chunks
    assert chunks(3, 65, 513, 33) >= 2 and chunks(3, 65, 256, 33) == 1 and chunks(1, 5, 1, 2) == 1
    for G, Mt in ((1, 100), (10, 200), (3, 256)):
        big = [ws(G, Mt, N, 8) for N in (10 ** 6, 10 ** 7, 2 * 10 ** 9)]
        assert min(big) > 0 and max(big) <= 1.05 * min(big)               # (the chunk length is rounded to 64 columns)
        for N in (1, 1000, 10 ** 6, 2 * 10 ** 9):
            n = chunks(G, Mt, N, 8)
            assert 1 <= n <= 1024 and n <= (N + 255) // 256
            assert ws(G, Mt, N, 8) <= n * G * (((Mt + 63) // 64) * 256 + 32) + 1024
    assert ws(0, 5, 5, 5) == 0 and chunks(1, 0, 5, 5) == 0
    assert ops.site_moments_chunks(3, 65, 513, 33) == chunks(3, 65, 513, 33) and ops.SITE_MAX_MT == 256


def test_site_cabi_argument_errors_before_any_launch():
    """A null pointer other than w (and log_scale unless Student-t), a size < 1, Mt above the LDS limit, an unknown kind or nu2, a
    bad ldy or df, a short workspace: VARGP_EINVAL (-1) with host memory for pointers -- nothing is launched."""
    from vargp_amd._lib import lib
    L = lib()
    EINVAL = -1
    G, Mt, N, D = 2, 5, 9, 3
    need = L.vargp_site_moments_workspace_bytes(G, Mt, N, D)
    buf = (ctypes.c_double * (need // 8 + 16))()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)

    def call(ptrs=None, ldy=N, w=p, kind=0, log_scale=p, df=4.0, outs=None, dims=(G, Mt, N, D), nu2=0, ws=p, ws_bytes=need):
        ptrs, outs = ptrs or [p] * 6, outs or [p] * 3
        return L.vargp_site_moments(*ptrs, ldy, w, kind, log_scale, df, 0.0, *outs, *dims, nu2, ws, ws_bytes, None)

    for bad in range(6):
        assert call(ptrs=[null if q == bad else p for q in range(6)]) == EINVAL
    for bad in range(3):
        assert call(outs=[null if q == bad else p for q in range(3)]) == EINVAL
    assert call(ws=null) == EINVAL
    for dims in ((0, Mt, N, D), (G, 0, N, D), (G, Mt, 0, D), (G, Mt, N, 0), (65536, Mt, N, D), (G, 257, N, D)):
        assert call(dims=dims, ws_bytes=1 << 40) == EINVAL, dims
    for kind in (-1, 4):
        assert call(kind=kind) == EINVAL
    for nu2 in (-1, 2, 4, 6):
        assert call(nu2=nu2) == EINVAL
    assert call(ldy=N - 1) == EINVAL and call(ldy=-1) == EINVAL
    assert call(kind=3, log_scale=null) == EINVAL and call(kind=3, df=0.0) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and call(ws_bytes=0) == EINVAL
    assert b'site_moments' in L.vargp_last_error()


# -- the Python surface -------------------------------------------------------------------------------------------------------------
def test_fit_q_newton_names_what_it_supports():
    from vargp_amd._lib import VargpHipError
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    labels = torch.arange(40) % 3
    with pytest.raises(ValueError, match='couples the outputs'):
        VARGP.create_clf(_Data(x, labels), M=4).fit_q_newton_(x, labels)
    reg = _Data(x, x[:, 0].clone())
    with pytest.raises(ValueError, match='fit_q_'):
        VARGP.create_reg(reg, M=4).fit_q_newton_(x, reg.targets)
    counts = _Data(x, torch.arange(40).float() % 4)
    with pytest.raises(ValueError, match='ep_var_mean=True'):
        VARGP.create_reg(counts, M=4, likelihood='poisson', ep_var_mean=False).fit_q_newton_(x, counts.targets)
    bern = VARGP.create_clf(_Data(x, labels), M=4, likelihood='bernoulli')
    for damping in (0.0, -0.5, 1.5, float('nan')):
        with pytest.raises(ValueError, match='damping'):
            bern.fit_q_newton_(x, labels, damping=damping)
    with pytest.raises(VargpHipError):                            # a supported model on the host: no CPU path
        bern.fit_q_newton_(x, labels)


def test_factories_refuse_newton_where_it_does_not_apply():
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    labels = torch.arange(40) % 3
    with pytest.raises(ValueError, match='q_init'):
        VARGP.create_clf(_Data(x, labels), M=4, q_init='best')
    with pytest.raises(ValueError, match='bernoulli'):
        VARGP.create_clf(_Data(x, labels), M=4, q_init='newton')                     # softmax
    reg = _Data(x, x[:, 0].clone())
    with pytest.raises(ValueError, match="'optimal'"):
        VARGP.create_reg(reg, M=4, q_init='newton')                                  # gaussian
    for q_init in ('optimal', 'collapsed'):
        with pytest.raises(ValueError, match='gaussian'):
            VARGP.create_reg(reg, M=4, likelihood='studentt', q_init=q_init)


def test_route_selection(monkeypatch):
    from vargp_amd import ops, sites
    monkeypatch.delenv('VARGP_SITES_ROUTE', raising=False)
    assert sites.pick_route(None, 256) == 'fused' and sites.pick_route(None, 257) == 'composed'
    assert sites.pick_route('composed', 10) == 'composed'
    with pytest.raises(ValueError, match='route'):
        sites.pick_route('fastest', 10)
    with pytest.raises(ValueError, match=str(ops.SITE_MAX_MT)):
        sites.pick_route('fused', 257)
    monkeypatch.setenv('VARGP_SITES_ROUTE', 'composed')
    assert sites.pick_route(None, 10) == 'composed' and sites.pick_route('fused', 10) == 'fused'


def test_ell_torch_is_the_restatement():
    """sites.ell_torch (the composed route's value) against ref_ell, every kind, including var = 0."""
    from vargp_amd import ops, sites
    g = torch.Generator().manual_seed(3)
    mu, var = torch.randn(2, 7, generator=g, dtype=F64), torch.rand(2, 7, generator=g, dtype=F64)
    var[0, 0] = 0.0
    yb, yc, yr = (torch.rand(2, 7, generator=g) < 0.5).double(), torch.poisson(torch.ones(2, 7) * 2.0, generator=g).double(), mu + 1.0
    ls = torch.tensor([-1.0, 0.3])
    cases = (('probit', {}, 'bernoulli', (0,), yb), ('logit', {}, 'bernoulli', (1,), yb), ('poisson', {}, 'poisson', (), yc),
             ('studentt', dict(log_scale=ls, df=3.0), 'studentt', (ls, 3.0, ops.studentt_lognorm(3.0)), yr))
    for kind, par, okind, extra, y in cases:
        assert torch.allclose(sites.ell_torch(okind, extra, mu, var, y), ref_ell(kind, par, mu, var, y), rtol=1e-12, atol=1e-13), kind
