"""The leave-one-out cavity (vargp_amd/loo.py, VARGP.loo), the part that needs no GPU: a dense fp64 restatement `ref_cavity` of the
formulas -- what tests/test_hip_loo.py measures the device against -- checked against brute force: for a Gaussian likelihood the
cavity moments ARE the moments at x_n of the closed-form q refitted with w_n = 0 (first task and with a frozen block: the
definition of s_n is what a frozen block tests); for probit they are the EP / CVI approximation of N refits.  Then the
zero-weight point, the unstable points of a q off the fixed point, the refusals of loo() and the C ABI of vargp_site_cavity.

Probit, N = 40, M = 10, converged ref_newton (tol 1e-12), as test_probit_is_closer_to_brute_force_than_in_sample printed it:
sum loo -13.3045, sum brute force -13.2951, sum in-sample -11.0736; max per-point |loo - brute| 9.2e-3; min r_n 0.766.
Gaussian identity: worst relative difference to the refits 7e-13 (first task), 5e-11 (with a frozen block)."""
import ctypes
import math

import pytest
import torch

from test_collapsed import _Data, make_problem, ref_fit, ref_kernel, ref_whiten
from test_sites_host import default_q, make_targets, ref_ell_derivs, ref_newton

F64 = torch.float64


# -- the restatement ----------------------------------------------------------------------------------------------------------------
def _cavity_from(kind, par, mu, var, s, y, w, eps=None):
    """Sites (the formulas of test_sites_host.ref_sites / test_softmax_sites_host.ref_softmax_sites) and cavity at given fp64
    marginals mu, var and shares s (G, N)."""
    if kind == 'softmax':
        from test_softmax_sites_host import ref_softmax_sites
        st = ref_softmax_sites(mu, var, y, w, eps)
        lam1, lam2 = st['lam1'], st['lam2']
        on = torch.ones_like(mu, dtype=torch.bool) if w is None else (w != 0).expand_as(mu)
    else:
        y64 = y.to(F64).expand(mu.shape[0], -1)
        w64 = torch.ones_like(mu) if w is None else w.to(F64)
        on, zero = w64 != 0, torch.zeros_like(mu)
        _, dmu, dvar = ref_ell_derivs(kind, par, mu, var, y64)
        lam2 = torch.where(on, w64 * (-2.0 * dvar).clamp_min(0.0), zero)
        lam1 = torch.where(on, w64 * dmu + lam2 * mu, zero)
    r = 1.0 - lam2 * s
    mu_c, var_c = (mu - s * lam1) / r, var + lam2 * s * s / r
    unstable = on & (~(r > 0) | ~torch.isfinite(mu_c) | ~torch.isfinite(var_c))
    return dict(mu=mu, var=var, s=s, lam1=lam1, lam2=lam2, r=r, mu_c=mu_c, var_c=var_c, unstable=unstable,
                n_unstable=unstable.sum(-1))


def ref_cavity_ops(kind, par, theta, Z, X, alpha, Q, V, y, w, nu2, eps=None):
    """ops.site_cavity dense in fp64, from the operands it takes: Z (G, Mt, D), X (N, D), alpha (G, Mt), Q (G, Mt, Mt), V (G, Mv,
    Mt), y (G, N) or (N,), w (G, N) or None; kind as test_sites_host names it ('gauss': par = dict(beta)), or 'softmax' with y (N,)
    int64, w (N,) or None and the noise eps (F, G, N).  -> dict(mu, var, s, lam1, lam2, r, mu_c, var_c (G, N), unstable (G, N)
    bool, n_unstable (G,)); the unstable points keep their raw moments here."""
    theta, Z, X, alpha, Q, V = (t.to(F64) for t in (theta, Z, X, alpha, Q, V))
    K = ref_kernel(Z, X.unsqueeze(0), theta, nu2)                                   # (G, Mt, N)
    mu = (alpha.unsqueeze(-1) * K).sum(-2)
    var = ((2.0 * theta[-1]).exp() - (K * (Q @ K)).sum(-2)).clamp_min(0.0)
    return _cavity_from(kind, par, mu, var, ((V @ K) ** 2).sum(-2), y, w, eps)


def ref_cavity(kind, par, theta, z_all, prev, x, y, w, nu2, a_t, H_t, eps=None):
    """loo.loo's moments dense in fp64 for q(v_t) = N(a_t, H_t H_t^T): z_all, prev as ref_whiten takes them.  The marginals and s
    from p_n = T k_n (|p_n|^2 <= gamma^2) rather than through alpha, Q and V, whose entries grow with |T|^2: the same numbers
    without the cancellation.  -> ref_cavity_ops' dict."""
    L, T, a_lt, H = ref_whiten(theta, z_all, prev, nu2)
    C, Mt = z_all.shape[:2]
    n_lt = Mt - a_t.shape[-1]
    a_t, H_t, theta = a_t.to(F64), H_t.to(F64), theta.to(F64)
    P = T @ ref_kernel(z_all.to(F64), x.to(F64).unsqueeze(0), theta, nu2)         # (C, Mt, N)
    Hb = torch.stack([torch.block_diag(*[Hi[c] for Hi in H], H_t[c]) for c in range(C)])
    mu = (P * torch.cat([a_lt, a_t], -1).unsqueeze(-1)).sum(-2)
    var = (((Hb.mT @ P) ** 2).sum(-2) + (2.0 * theta[-1]).exp() - (P * P).sum(-2)).clamp_min(0.0)
    return _cavity_from(kind, par, mu, var, ((H_t.mT @ P[:, n_lt:]) ** 2).sum(-2), y, w, eps)


def ref_moments_at(theta, z_all, prev, x, nu2, a_t, Sigma_t):
    """mu, var (C, N) of q(f) at x for q(v_t) = N(a_t, Sigma_t), dense fp64."""
    L, T, a_lt, H = ref_whiten(theta, z_all, prev, nu2)
    C = z_all.shape[0]
    P = T @ ref_kernel(z_all.to(F64), x.to(F64).unsqueeze(0), theta.to(F64), nu2)
    HH = torch.stack([torch.block_diag(*[Hi[c] @ Hi[c].mT for Hi in H], Sigma_t[c]) for c in range(C)])
    return (P * torch.cat([a_lt, a_t], -1).unsqueeze(-1)).sum(-2), \
        (P * (HH @ P)).sum(-2) + (2.0 * theta[-1].to(F64)).exp() - (P * P).sum(-2)


def _probit_lpd(mu, var, y):
    """log of the probit model's predictive probability of y in {0, 1}: the closed form Phi(s mu / sqrt(1 + var))."""
    return torch.special.log_ndtr((2.0 * y - 1.0) * mu / (1.0 + var).sqrt())


# -- the formulas against brute force -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('t,n_prev_pts', [(0, 0), (1, 6)])
def test_gaussian_cavity_is_the_refit_without_the_point(t, n_prev_pts):
    """N = 24, M = 8, D = 2, C = 2, weights; first task, and one previous task of 6 inducing points: for every n the cavity moments
    are the moments at x_n of ref_fit's closed-form q with w_n = 0, to fp64 rounding."""
    pr = make_problem(2, 8, 0, 2, 24, seed=50 + t, weights=True)
    if t:
        g = torch.Generator().manual_seed(77)
        pz = torch.randn(2, n_prev_pts, 2, generator=g)
        vec = 0.3 * torch.randn(2, n_prev_pts * (n_prev_pts + 1) // 2, generator=g)
        from test_collapsed import ref_vec2tril
        pr['prev'] = [dict(z=pz, u_mean=0.5 * torch.randn(2, n_prev_pts, 1, generator=g), u_tril_vec=vec,
                           u_tril=ref_vec2tril(vec, n_prev_pts))]
        pr['z_all'] = torch.cat([pz, pr['z_all']], -2)
    args = (pr['theta'], pr['z_all'], pr['prev'], pr['x'], pr['y'])
    fit = ref_fit(*args, pr['w'], pr['obs_log_var'], 0)
    H_t = torch.linalg.cholesky(fit['Sigma_t'])
    cav = ref_cavity('gauss', dict(beta=(-pr['obs_log_var'].double()).exp()), *args, pr['w'], 0, fit['a_t'], H_t)
    assert int(cav['n_unstable'].sum()) == 0 and cav['r'].min().item() > 0
    assert bool((cav['s'] >= 0).all()) and bool((cav['s'] <= cav['var'] * (1 + 1e-9)).all())
    worst = 0.0
    for n in range(24):
        w = pr['w'].clone()
        w[:, n] = 0.0
        out = ref_fit(*args, w, pr['obs_log_var'], 0)
        mu, var = ref_moments_at(pr['theta'], pr['z_all'], pr['prev'], pr['x'][n:n + 1], 0, out['a_t'], out['Sigma_t'])
        worst = max(worst, ((mu[:, 0] - cav['mu_c'][:, n]).abs() / mu[:, 0].abs().clamp_min(1.0)).max().item(),
                    ((var[:, 0] - cav['var_c'][:, n]).abs() / var[:, 0].abs()).max().item())
        assert torch.allclose(cav['mu_c'][:, n], mu[:, 0], rtol=1e-9, atol=1e-9), (n, cav['mu_c'][:, n], mu[:, 0])
        assert torch.allclose(cav['var_c'][:, n], var[:, 0], rtol=1e-9, atol=0.0), (n, cav['var_c'][:, n], var[:, 0])
    print(f't={t}: worst relative difference to the refits {worst:.2e}')


def test_probit_is_closer_to_brute_force_than_in_sample():
    """N = 40, M = 10, converged ref_newton; brute force: N refits with w_n = 0.  |sum loo - sum brute| < |sum in-sample - sum
    brute|, and r_n > 0 everywhere."""
    pr = make_problem(1, 10, 0, 2, 40, seed=60)
    y = make_targets('probit', pr, 7)
    u_mean0, u_tril0 = default_q(1, 10, 4)
    args = ('probit', {}, pr['theta'], pr['z_all'], pr['prev'], pr['x'], y)
    run = lambda w: ref_newton(*args, w, 0, u_mean0, u_tril0, n_iters=50, tol=1e-12)
    fit = run(None)
    assert fit['n_iters'] < 50
    H_t = torch.linalg.cholesky(fit['Sigma_t'])
    cav = ref_cavity(*args, None, 0, fit['a_t'], H_t)
    assert cav['r'].min().item() > 0 and int(cav['n_unstable'].sum()) == 0
    y64 = y.to(F64)
    loo = _probit_lpd(cav['mu_c'], cav['var_c'], y64)[0]
    insample = _probit_lpd(cav['mu'], cav['var'], y64)[0]
    brute = torch.empty(40, dtype=F64)
    for n in range(40):
        w = torch.ones(1, 40)
        w[0, n] = 0.0
        out = run(w)
        mu, var = ref_moments_at(pr['theta'], pr['z_all'], pr['prev'], pr['x'][n:n + 1], 0, out['a_t'], out['Sigma_t'])
        brute[n] = _probit_lpd(mu, var, y64[:, n:n + 1])[0, 0]
    print(f'probit: sum loo {loo.sum().item():.4f} brute {brute.sum().item():.4f} in-sample {insample.sum().item():.4f}; '
          f'max per-point |loo - brute| {(loo - brute).abs().max().item():.2e}; min r {cav["r"].min().item():.3f}')
    assert abs(loo.sum().item() - brute.sum().item()) < abs(insample.sum().item() - brute.sum().item())


def test_zero_weight_point_keeps_its_marginal():
    pr = make_problem(2, 5, 1, 3, 30, seed=61, weights=True)
    pr['w'][:, 4] = 0.0
    pr['w'][1, 9] = 0.0
    y = make_targets('logit', pr, 8)
    u_mean0, u_tril0 = default_q(2, 5, 5)
    fit = ref_newton('logit', {}, pr['theta'], pr['z_all'], pr['prev'], pr['x'], y, pr['w'], 0, u_mean0, u_tril0)
    cav = ref_cavity('logit', {}, pr['theta'], pr['z_all'], pr['prev'], pr['x'], y, pr['w'], 0, fit['a_t'],
                     torch.linalg.cholesky(fit['Sigma_t']))
    off = pr['w'] == 0
    assert int(off.sum()) == 3
    assert torch.equal(cav['mu_c'][off], cav['mu'][off]) and torch.equal(cav['var_c'][off], cav['var'][off])
    assert bool((cav['lam1'][off] == 0).all()) and bool((cav['lam2'][off] == 0).all()) and not bool(cav['unstable'][off].any())
    assert not torch.equal(cav['mu_c'][~off], cav['mu'][~off])


def test_a_q_off_the_fixed_point_has_unstable_points():
    """H_t of a converged probit fit scaled x 3: q is nine times as wide as "prior + sites" allows, lam2_n s_n exceeds 1 at the
    points whose site is strong, and exactly those are unstable: the restatement's r_n <= 0 defines the set."""
    pr = make_problem(2, 6, 0, 2, 50, seed=62)
    y = make_targets('probit', pr, 9)
    u_mean0, u_tril0 = default_q(2, 6, 6)
    args = ('probit', {}, pr['theta'], pr['z_all'], pr['prev'], pr['x'], y, None, 0)
    fit = ref_newton(*args, u_mean0, u_tril0)
    H_t = torch.linalg.cholesky(fit['Sigma_t'])
    good, bad = ref_cavity(*args, fit['a_t'], H_t), ref_cavity(*args, fit['a_t'], 3.0 * H_t)
    assert int(good['n_unstable'].sum()) == 0
    expect = ~(bad['r'] > 0)
    print(f'unstable per output {bad["n_unstable"].tolist()} of 50; r in [{bad["r"].min().item():.3f}, {bad["r"].max().item():.3f}]')
    assert torch.equal(bad['unstable'], expect) and torch.equal(bad['n_unstable'], expect.sum(-1))
    assert 0 < int(expect.sum()) < expect.numel()
    # a stable point's cavity is proper; an unstable point's raw variance is not
    assert bool((bad['var_c'][~expect] >= bad['var'][~expect]).all()) and bool((bad['var_c'][expect] < bad['var'][expect]).all())


def test_cavity_torch_is_the_restatement():
    """loo.cavity_torch (the elementwise step of the Gaussian and softmax routes) on host tensors: the formulas, NaN exactly at
    the unstable points, the count, and an exact marginal where the site is zero."""
    from vargp_amd.loo import cavity_torch
    g = torch.Generator().manual_seed(4)
    mu, var, s = torch.randn(2, 9, generator=g), torch.rand(2, 9, generator=g) + 0.5, torch.rand(2, 9, generator=g) * 0.5
    lam1, lam2 = torch.randn(2, 9, generator=g), torch.rand(2, 9, generator=g)
    s[1, 5], lam2[0, 3], lam2[1, 5] = 0.25, 4.0 / s[0, 3], 4.0                      # r = -3 and r = 0 exactly
    lam1[1, 0] = lam2[1, 0] = 0.0
    mu_c, var_c, n_un = cavity_torch(mu, var, s, lam1, lam2)
    r = 1.0 - lam2.double() * s.double()
    bad = ~(r > 0)
    assert n_un.tolist() == [1, 1] and bad.sum().item() == 2
    assert torch.equal(torch.isnan(mu_c), bad) and torch.equal(torch.isnan(var_c), bad)
    assert torch.equal(mu_c[~bad], ((mu.double() - s.double() * lam1.double()) / r).float()[~bad])
    assert torch.equal(var_c[~bad], (var.double() + lam2.double() * s.double() ** 2 / r).float()[~bad])
    assert mu_c[1, 0].item() == mu[1, 0].item() and var_c[1, 0].item() == var[1, 0].item()


# -- the Python surface -------------------------------------------------------------------------------------------------------------
def test_loo_names_what_it_supports():
    from vargp_amd import loo
    from vargp_amd._lib import VargpHipError
    from vargp_amd.kernels import RBFKernel
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    labels = torch.arange(40) % 3
    counts = _Data(x, torch.arange(40).float() % 4)
    with pytest.raises(ValueError, match='ep_var_mean=True'):
        VARGP.create_reg(counts, M=4, likelihood='poisson', ep_var_mean=False).loo(x, counts.targets)
    with pytest.raises(ValueError, match='ep_var_mean=True'):
        VARGP.create_clf(_Data(x, labels), M=4, ep_var_mean=False).loo(x, labels)

    class OtherKernel(torch.nn.Module):
        log_mean = torch.zeros(4)

    gp = VARGP.create_clf(_Data(x, labels), M=4, likelihood='bernoulli')
    gp.kernel = OtherKernel()
    with pytest.raises(ValueError, match='supported kernels'):
        gp.loo(x, labels)
    gp = VARGP.create_clf(_Data(x, labels), M=4, likelihood='bernoulli')
    gp.likelihood = torch.nn.Identity()
    with pytest.raises(ValueError, match='supported likelihoods'):
        loo.check_supported(gp)
    # every likelihood of the project is accepted, and a supported model on the host has no CPU path
    reg = _Data(x, x[:, 0].clone())
    for gp, y in ((VARGP.create_clf(_Data(x, labels), M=4), labels), (VARGP.create_clf(_Data(x, labels), M=4, likelihood='bernoulli'), labels),
                  (VARGP.create_reg(reg, M=4), reg.targets), (VARGP.create_reg(reg, M=4, likelihood='studentt'), reg.targets),
                  (VARGP.create_reg(counts, M=4, likelihood='poisson'), counts.targets)):
        loo.check_supported(gp)
        with pytest.raises(VargpHipError):
            gp.loo(x, y)
    with pytest.raises(ValueError, match='tile'):
        VARGP.create_reg(reg, M=4).loo(x, reg.targets, tile=0)
    with pytest.raises(ValueError, match='n_f'):
        VARGP.create_clf(_Data(x, labels), M=4).loo(x, labels, n_f=0)


# -- the C ABI ----------------------------------------------------------------------------------------------------------------------
CAVITY_SYMBOLS = ('vargp_site_cavity', 'vargp_site_cavity_workspace_bytes', 'vargp_site_cavity_chunks')


def test_cavity_symbols_are_exported_and_declared():
    import os
    import re
    from conftest import ROOT
    from vargp_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vargp_hip.h')).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in CAVITY_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(handle, name) and hasattr(_lib.lib(), name)
        assert re.search(r'\b%s\s*\(' % name, text), f'{name} is not declared in include/vargp_hip.h'


def test_cavity_workspace_and_chunks():
    """The chunking is site_moments'; the workspace holds one double per (output, chunk) and does not grow with N beyond that."""
    from vargp_amd import ops
    from vargp_amd._lib import lib
    ws, chunks = lib().vargp_site_cavity_workspace_bytes, lib().vargp_site_cavity_chunks
    for G, Mt, N, D in ((3, 65, 513, 33), (1, 5, 1, 2), (10, 200, 10 ** 6, 8), (3, 256, 2 * 10 ** 9, 8)):
        n = chunks(G, Mt, N, D)
        assert n == lib().vargp_site_moments_chunks(G, Mt, N, D) and 1 <= n <= 1024
        assert 8 * G * n <= ws(G, Mt, N, D) <= 8 * G * n + 512
    assert ws(0, 5, 5, 5) == 0 and chunks(1, 0, 5, 5) == 0
    assert ops.site_cavity_chunks(3, 65, 513, 33) == chunks(3, 65, 513, 33) >= 2


def test_cavity_cabi_argument_errors_before_any_launch():
    """Host memory for every pointer: VARGP_EINVAL (-1) and nothing is launched.  Both forms need theta, Z, X, alpha, Q, V, mu,
    var, s; the site form (kind >= 0) also y, the other five outputs and the workspace; Mt <= 256; 1 <= Mv <= Mt."""
    from vargp_amd._lib import lib
    L = lib()
    EINVAL = -1
    G, Mt, Mv, N, D = 2, 5, 3, 9, 3
    need = L.vargp_site_cavity_workspace_bytes(G, Mt, N, D)
    buf = (ctypes.c_double * (need // 8 + 16))()
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)

    def call(ins=None, y=p, ldy=N, w=p, kind=0, log_scale=p, df=4.0, outs=None, dims=(G, Mt, Mv, N, D), nu2=0, ws=p, ws_bytes=need):
        ins, outs = ins or [p] * 6, outs or [p] * 8
        return L.vargp_site_cavity(*ins, y, ldy, w, kind, log_scale, df, 0.0, *outs, *dims, nu2, ws, ws_bytes, None)

    for kind in (0, -1):
        for bad in range(6):
            assert call(ins=[null if q == bad else p for q in range(6)], kind=kind) == EINVAL
        for bad in range(3):
            assert call(outs=[null if q == bad else p for q in range(8)], kind=kind) == EINVAL
        for dims in ((0, Mt, Mv, N, D), (G, 0, Mv, N, D), (G, Mt, Mv, 0, D), (G, Mt, Mv, N, 0), (65536, Mt, Mv, N, D),
                     (G, 257, Mv, N, D), (G, Mt, 0, N, D), (G, Mt, Mt + 1, N, D), (G, 256, 257, N, D)):
            assert call(dims=dims, kind=kind, ws_bytes=1 << 40) == EINVAL, (kind, dims)
        for nu2 in (-1, 2, 4, 6):
            assert call(nu2=nu2, kind=kind) == EINVAL
    for bad in range(3, 8):
        assert call(outs=[null if q == bad else p for q in range(8)]) == EINVAL
    assert call(y=null) == EINVAL and call(ws=null) == EINVAL and call(kind=4) == EINVAL
    assert call(ldy=N - 1) == EINVAL and call(ldy=-1) == EINVAL
    assert call(kind=3, log_scale=null) == EINVAL and call(kind=3, df=0.0) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and call(ws_bytes=0) == EINVAL
    assert b'site_cavity' in L.vargp_last_error()
