"""The natural-gradient q(u) fit for MulticlassSoftmax (vargp_amd/sites.py: fit_q_softmax_), the part that needs no GPU: a dense
fp64 restatement in plain torch of the softmax site pass (csrc/softmax_sites.hip) and of the whole iteration with explicit noise
-- what tests/test_hip_softmax_sites.py measures the device against -- checked against itself: at C = 2 the Monte-Carlo means of
1e5 draws are within 5 standard errors of a 2-D Gauss-Hermite product rule, lam2 >= 0 everywhere, and the accepted trace of the
iteration never falls.  Then the argument checks of the four new C-ABI entries and the ValueErrors of the Python surface."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_collapsed import _Data, ref_kernel, ref_whiten
from test_sites_host import _kl, _mv

F64 = torch.float64


# -- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_softmax_sites(mu, var, y, w, eps):
    """One softmax site pass, fp64 (the formulas of csrc/softmax_sites.hip).  mu, var (C, N), y (N,) int64, w (N,) or None, eps
    (F, C, N) -> dict(lam1, lam2 (C, N), sums (4,), ell (N,), Ep, Ev (C, N), se: the standard errors of ell, Ep, Ev)."""
    mu, var, eps = mu.to(F64), var.to(F64), eps.to(F64)
    C, N = mu.shape
    F = eps.shape[0]
    f = mu + var.sqrt() * eps
    lse = torch.logsumexp(f, -2)                                                     # (F, N)
    p = torch.softmax(f, -2)
    v = p * (1.0 - p)
    hot = (y.unsqueeze(0) == torch.arange(C).unsqueeze(1)).to(F64)
    ell = (mu * hot).sum(0) - lse.mean(0)
    Ep, Ev = p.mean(0), v.mean(0)
    w = torch.ones(N, dtype=F64) if w is None else w.to(F64)
    on, zero = w != 0, torch.zeros_like(mu)
    lam2 = torch.where(on, w * Ev, zero)
    lam1 = torch.where(on, w * (hot - Ep) + lam2 * mu, zero)
    sums = torch.stack([torch.where(on, w * ell, torch.zeros_like(ell)).sum(), lam2.sum(), on.to(F64).sum(), w.sum()])
    se = None if F < 2 else dict(ell=lse.std(0) / math.sqrt(F), Ep=p.std(0) / math.sqrt(F), Ev=v.std(0) / math.sqrt(F))
    return dict(lam1=lam1, lam2=lam2, sums=sums, ell=ell, Ep=Ep, Ev=Ev, se=se)


def ref_softmax_newton(theta, z_all, prev, x, y, w, nu2, u_mean0, u_tril0, eps, n_iters=20, damping=1.0, tol=1e-6, max_halvings=8):
    """sites.fit_q_softmax_ restated dense in fp64 with the explicit noise eps (F, C, N).  Arguments as test_sites_host.ref_newton
    takes them; y (N,) int64, w (N,) or None.  A candidate is judged on the bound summed over the classes.  -> dict(u_mean (C, M),
    S_u (C, M, M) = L_u L_u^T, a_t, Sigma_t, trace (n + 1, 1), n_iters, n_rejected, decisions: [(accepted, (candidate - parent)
    / |parent|)] of every candidate in order, mu, var: the marginals at the final q)."""
    L, T, a_lt, H = ref_whiten(theta, z_all, prev, nu2)
    C, Mt = z_all.shape[:2]
    M = u_mean0.shape[-2]
    n_lt = Mt - M
    T_tt, L_tt = T[:, n_lt:, n_lt:], L[:, n_lt:, n_lt:]
    eye = torch.eye(M, dtype=F64)
    th = theta.to(F64)
    K = ref_kernel(z_all.to(F64), x.to(F64).unsqueeze(0), th, nu2)                  # (C, Mt, N)
    g2 = (2.0 * th[-1]).exp()

    def sites_at(a_t, Sigma):
        a = torch.cat([a_lt, a_t], -1)
        HH = torch.stack([torch.block_diag(*[(Hi[c] @ Hi[c].mT) for Hi in H], Sigma[c]) for c in range(C)])
        Q = T.mT @ (torch.eye(Mt, dtype=F64) - HH) @ T
        Q = 0.5 * (Q + Q.mT)
        mu = (_mv(T.mT, a).unsqueeze(-1) * K).sum(-2)
        var = (g2 - (K * (Q @ K)).sum(-2)).clamp_min(0.0)
        s = ref_softmax_sites(mu, var, y, w, eps)
        A = T @ ((K * s['lam2'].unsqueeze(-2)) @ K.mT) @ T.mT
        tc = _mv(T, (K * s['lam1'].unsqueeze(-2)).sum(-1))
        bound = (s['sums'][0] - _kl(a_t, Sigma).sum()).view(1)
        return bound, eye + A[:, n_lt:, n_lt:], tc[:, n_lt:] - _mv(A[:, n_lt:, :n_lt], a_lt), (mu, var)

    a_t = _mv(T_tt, u_mean0.to(F64).squeeze(-1))
    H_t = T_tt @ u_tril0.to(F64)
    Sigma = H_t @ H_t.mT
    P = torch.linalg.inv(Sigma)
    P = 0.5 * (P + P.mT)
    h = _mv(P, a_t)
    bound, P_new, h_new, marg = sites_at(a_t, Sigma)
    trace, n_rejected, decisions = [bound], 0, []
    while len(trace) - 1 < n_iters:
        rho, accepted = damping, None
        for _ in range(max_halvings + 1):
            P_c, h_c = (1.0 - rho) * P + rho * P_new, (1.0 - rho) * h + rho * h_new
            S_c = torch.linalg.inv(P_c)
            S_c = 0.5 * (S_c + S_c.mT)
            a_c = _mv(S_c, h_c)
            bound_c, P_next, h_next, marg_c = sites_at(a_c, S_c)
            ok = bool(torch.isfinite(bound_c).all()) and bool((bound_c >= trace[-1]).all())
            decisions.append((ok, ((bound_c - trace[-1]) / trace[-1].abs()).item()))
            if ok:
                accepted = (P_c, h_c, a_c, S_c, P_next, h_next, marg_c)
                break
            n_rejected += 1
            rho *= 0.5
        if accepted is None:
            break
        P, h, a_t, Sigma, P_new, h_new, marg = accepted
        trace.append(bound_c)
        if (trace[-1].sum() - trace[-2].sum()).item() < tol * abs(trace[-1].sum().item()):
            break
    S_u = L_tt @ Sigma @ L_tt.mT
    return dict(u_mean=_mv(L_tt, a_t), S_u=0.5 * (S_u + S_u.mT), a_t=a_t, Sigma_t=Sigma, trace=torch.stack(trace),
                n_iters=len(trace) - 1, n_rejected=n_rejected, decisions=decisions, mu=marg[0], var=marg[1])


def blobs(C, N, D, seed, radius=4.0, turn=0.0):
    """C unit-variance Gaussian blobs, their centres evenly on a circle of `radius` in the first two of D >= 2 dimensions (three
    blobs: 6.9 standard deviations apart, so the classes overlap in well under 1 % of the points), the circle turned by `turn`
    of a full turn -> x (N, D) float32, y (N,)"""
    g = torch.Generator().manual_seed(seed)
    ang = 2.0 * math.pi * (torch.arange(C) / C + turn)
    centres = torch.zeros(C, D)
    centres[:, 0], centres[:, 1] = radius * ang.cos(), radius * ang.sin()
    y = torch.arange(N) % C
    return (centres[y] + torch.randn(N, D, generator=g)).float(), y


# -- the restatement against itself -------------------------------------------------------------------------------------------------
def test_monte_carlo_means_against_gauss_hermite_at_two_classes():
    """C = 2: the exact ell, E p_c and E p_c (1 - p_c) from a 2-D product of 40-node Gauss-Hermite rules (the integrands are smooth
    and bounded by polynomials, the rule is exact to far below the standard errors here); the restatement with F = 1e5 draws is
    within 5 standard errors of each."""
    g = torch.Generator().manual_seed(1)
    N, F = 6, 100000
    mu = 1.5 * torch.randn(2, N, generator=g, dtype=F64)
    var = 0.2 + 1.5 * torch.rand(2, N, generator=g, dtype=F64)
    y = torch.arange(N) % 2
    eps = torch.randn(F, 2, N, generator=g, dtype=F64)
    got = ref_softmax_sites(mu, var, y, None, eps)
    xs, ws = np.polynomial.hermite.hermgauss(40)
    xs, ws = torch.tensor(xs, dtype=F64), torch.tensor(ws / math.sqrt(math.pi), dtype=F64)
    f0 = mu[0].view(N, 1, 1) + (2.0 * var[0]).sqrt().view(N, 1, 1) * xs.view(1, -1, 1)
    f1 = mu[1].view(N, 1, 1) + (2.0 * var[1]).sqrt().view(N, 1, 1) * xs.view(1, 1, -1)
    f = torch.stack([f0.expand(N, 40, 40), f1.expand(N, 40, 40)])                   # (2, N, 40, 40)
    w2 = ws.view(-1, 1) * ws.view(1, -1)
    E = lambda t: (t * w2).sum((-2, -1))
    p = torch.softmax(f, 0)
    ell = mu[y, torch.arange(N)] - E(torch.logsumexp(f, 0))
    Ep, Ev = E(p), E(p * (1.0 - p))
    for name, exact in (('ell', ell), ('Ep', Ep), ('Ev', Ev)):
        z = ((got[name] - exact) / got['se'][name]).abs().max().item()
        print(f'{name}: largest deviation {z:.2f} standard errors')
        assert z < 5.0, (name, z)
    assert torch.allclose(Ep.sum(0), torch.ones(N, dtype=F64), atol=1e-12)


def test_lam2_is_never_negative_and_zero_weights_add_nothing():
    g = torch.Generator().manual_seed(2)
    C, N, F = 5, 40, 3
    mu, var = 4.0 * torch.randn(C, N, generator=g), torch.rand(C, N, generator=g)
    mu[0, :5], mu[1, :5] = 60.0, -60.0
    var[:, 7] = 0.0
    y = torch.randint(0, C, (N,), generator=g)
    w = torch.rand(N, generator=g)
    w[::3] = 0.0
    eps = torch.randn(F, C, N, generator=g)
    a = ref_softmax_sites(mu, var, y, w, eps)
    assert bool((a['lam2'] >= 0).all()) and bool(torch.isfinite(a['lam1']).all()) and bool(torch.isfinite(a['sums']).all())
    assert bool((a['lam1'][:, ::3] == 0).all()) and bool((a['lam2'][:, ::3] == 0).all())
    mu2, y2 = mu.clone(), y.clone()
    mu2[:, ::3], y2[::3] = 1e3, 0
    b = ref_softmax_sites(mu2, var, y2, w, eps)
    assert torch.equal(a['sums'], b['sums']) and torch.equal(a['lam1'], b['lam1'])
    assert a['sums'][2].item() == float((w != 0).sum()) and a['sums'][3].item() == pytest.approx(w.double().sum().item())


@pytest.mark.parametrize('n_f,start', [(32, 'prior'), (1, 'prior'), (8, 'default')])
def test_restated_trace_never_falls(n_f, start):
    """Three blobs, M = 8: the accepted trace is non-decreasing with common random numbers, also with one draw per point and from
    the wide default q; the fit classifies the blobs."""
    C, N, D, M = 3, 90, 2, 8
    x, y = blobs(C, N, D, 3)
    g = torch.Generator().manual_seed(4)
    z = torch.stack([x[torch.randperm(N, generator=g)[:M]] for _ in range(C)])
    theta = torch.cat([torch.full((D,), math.log(1.5)), torch.tensor([0.0])])
    if start == 'prior':
        u_mean0, u_tril0 = torch.zeros(C, M, 1), ref_whiten(theta, z, [], 0)[0]
    else:
        u_mean0, u_tril0 = 0.5 * torch.randn(C, M, 1, generator=g), math.log1p(math.e) * torch.eye(M).expand(C, M, M)
    eps = torch.randn(n_f, C, N, generator=g, dtype=F64)
    got = ref_softmax_newton(theta, z, [], x, y, None, 0, u_mean0, u_tril0, eps)
    tr = got['trace']
    print(f'F = {n_f} {start}: {got["n_iters"]} accepted, {got["n_rejected"]} rejected, trace {tr.view(-1).tolist()}')
    assert tuple(tr.shape) == (got['n_iters'] + 1, 1) and got['n_iters'] >= 1
    assert bool((tr[1:] >= tr[:-1]).all()) and tr[-1].item() > tr[0].item()
    assert (got['mu'].argmax(0) == y).double().mean().item() >= 0.9


# -- the C ABI ----------------------------------------------------------------------------------------------------------------------
EINVAL = -1


def _host_buffer(nbytes):
    buf = (ctypes.c_double * (nbytes // 8 + 16))()
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_new_symbols_are_exported():
    from vargp_amd import _lib
    for name in ('vargp_site_marginals', 'vargp_softmax_sites', 'vargp_softmax_sites_workspace_bytes', 'vargp_softmax_site_noise',
                 'vargp_gram_moments_v'):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)


def test_site_marginals_argument_errors_before_any_launch():
    from vargp_amd._lib import lib
    L = lib()
    buf, p = _host_buffer(1024)
    null = ctypes.c_void_p(0)
    call = lambda ptrs=None, dims=(2, 5, 9, 3), nu2=0: L.vargp_site_marginals(*(ptrs or [p] * 7), *dims, nu2, None)
    for bad in range(7):
        assert call(ptrs=[null if q == bad else p for q in range(7)]) == EINVAL
    for dims in ((0, 5, 9, 3), (2, 0, 9, 3), (2, 5, 0, 3), (2, 5, 9, 0), (65536, 5, 9, 3), (2, 257, 9, 3)):
        assert call(dims=dims) == EINVAL, dims
    for nu2 in (-1, 2, 4, 6):
        assert call(nu2=nu2) == EINVAL
    assert b'site_marginals' in L.vargp_last_error()


def test_softmax_sites_argument_errors_before_any_launch():
    from vargp_amd import ops
    from vargp_amd._lib import lib
    L = lib()
    C, N, F = 3, 9, 2
    need = L.vargp_softmax_sites_workspace_bytes(C, N)
    assert need > 0 and L.vargp_softmax_sites_workspace_bytes(0, N) == 0 and L.vargp_softmax_sites_workspace_bytes(C, 0) == 0
    # per-chunk partials only: at most 1024 chunks of 32 bytes, whatever N is
    assert L.vargp_softmax_sites_workspace_bytes(10, 2 * 10 ** 9) <= 1024 * 32 + 256
    buf, p = _host_buffer(need)
    null = ctypes.c_void_p(0)

    def call(mu=p, var=p, y=p, w=p, eps=p, outs=None, dims=(C, N, F), ws=p, ws_bytes=need):
        return L.vargp_softmax_sites(mu, var, y, w, eps, 0, *(outs or [p] * 3), *dims, ws, ws_bytes, None)

    assert call(mu=null) == EINVAL and call(var=null) == EINVAL and call(y=null) == EINVAL and call(ws=null) == EINVAL
    for bad in range(3):
        assert call(outs=[null if q == bad else p for q in range(3)]) == EINVAL
    for dims in ((1, N, F), (0, N, F), (C, 0, F), (C, N, 0), (C, N, 65536)):
        assert call(dims=dims) == EINVAL, dims
    assert call(dims=(129, N, F), ws_bytes=1 << 30) == EINVAL
    assert b'128' in L.vargp_last_error() and b'softmax_sites' in L.vargp_last_error()
    assert call(ws_bytes=need - 1) == EINVAL and call(ws_bytes=0) == EINVAL
    assert call(ws=ctypes.c_void_p(p.value + 4)) == EINVAL                          # misaligned
    assert ops.SOFTMAX_SITE_MAX_C == 128


def test_softmax_site_noise_argument_errors_before_any_launch():
    from vargp_amd._lib import lib
    L = lib()
    buf, p = _host_buffer(1024)
    assert L.vargp_softmax_site_noise(0, ctypes.c_void_p(0), 2, 3, 9, None) == EINVAL
    for dims in ((0, 3, 9), (2, 1, 9), (2, 129, 9), (2, 3, 0), (65536, 3, 9)):
        assert L.vargp_softmax_site_noise(0, p, *dims, None) == EINVAL, dims
    assert b'softmax_site_noise' in L.vargp_last_error()


def test_gram_moments_v_argument_errors_before_any_launch():
    from vargp_amd._lib import lib
    L = lib()
    G, Mt, N, D = 2, 5, 9, 3
    need = L.vargp_gram_moments_workspace_bytes(G, Mt, N, D)
    buf, p = _host_buffer(need)
    null = ctypes.c_void_p(0)

    def call(ptrs=None, dims=(G, Mt, N, D), nu2=0, ws=p, ws_bytes=need):
        return L.vargp_gram_moments_v(*(ptrs or [p] * 8), *dims, nu2, ws, ws_bytes, None)

    for bad in (0, 1, 2, 4, 5, 6, 7):                                                # (3 is w: optional)
        assert call(ptrs=[null if q == bad else p for q in range(8)]) == EINVAL, bad
    assert call(ws=null) == EINVAL
    for dims in ((0, Mt, N, D), (G, 0, N, D), (G, Mt, 0, D), (G, Mt, N, 0), (65536, Mt, N, D)):
        assert call(dims=dims, ws_bytes=1 << 40) == EINVAL, dims
    for nu2 in (-1, 2, 4, 6):
        assert call(nu2=nu2) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL
    assert b'gram_moments_v' in L.vargp_last_error()


# -- the Python surface -------------------------------------------------------------------------------------------------------------
def test_fit_q_softmax_names_what_it_supports():
    from vargp_amd._lib import VargpHipError
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    labels = torch.arange(40) % 3
    data = _Data(x, labels)
    with pytest.raises(ValueError, match='MulticlassSoftmax'):
        VARGP.create_clf(data, M=4, likelihood='bernoulli').fit_q_softmax_(x, labels)
    counts = _Data(x, torch.arange(40).float() % 4)
    with pytest.raises(ValueError, match='MulticlassSoftmax'):
        VARGP.create_reg(counts, M=4, likelihood='poisson').fit_q_softmax_(x, labels)
    with pytest.raises(ValueError, match='ep_var_mean=True'):
        VARGP.create_clf(data, M=4, ep_var_mean=False).fit_q_softmax_(x, labels)
    gp = VARGP.create_clf(data, M=4)
    with pytest.raises(ValueError, match='weights'):
        gp.fit_q_softmax_(x, labels, weights=torch.ones(3, 40))
    for damping in (0.0, -0.5, 1.5, float('nan')):
        with pytest.raises(ValueError, match='damping'):
            gp.fit_q_softmax_(x, labels, damping=damping)
    with pytest.raises(ValueError, match='start'):
        gp.fit_q_softmax_(x, labels, start='best')
    for n_f in (0, -1, 65536):
        with pytest.raises(ValueError, match='n_f'):
            gp.fit_q_softmax_(x, labels, n_f=n_f)
    with pytest.raises(VargpHipError):                            # a supported model on the host: no CPU path
        gp.fit_q_softmax_(x, labels)
    with pytest.raises(ValueError, match='couples the outputs'):  # the independent-output fit still refuses the softmax
        gp.fit_q_newton_(x, labels)


def test_factory_refuses_newton_softmax_where_it_does_not_apply():
    from vargp_amd.vargp import VARGP, _CLF_Q_INITS
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    data = _Data(x, torch.arange(40) % 3)
    assert 'newton_softmax' in _CLF_Q_INITS
    with pytest.raises(ValueError, match="'newton'"):
        VARGP.create_clf(data, M=4, q_init='newton_softmax', likelihood='bernoulli')
    with pytest.raises(ValueError, match='bernoulli'):
        VARGP.create_clf(data, M=4, q_init='newton')              # softmax: unchanged


def test_ops_refuse_host_tensors():
    from vargp_amd import ops, sites
    from vargp_amd._lib import VargpHipError
    mu = torch.zeros(3, 5)
    with pytest.raises(VargpHipError):
        ops.softmax_sites(mu, mu, torch.zeros(5, dtype=torch.int64), None, 2)
    with pytest.raises(VargpHipError):
        ops.site_marginals(torch.zeros(3), torch.zeros(3, 4, 2), torch.zeros(5, 2), torch.zeros(3, 4), torch.zeros(3, 4, 4))
    with pytest.raises(VargpHipError):
        ops.gram_moments_v(torch.zeros(3), torch.zeros(3, 4, 2), torch.zeros(5, 2), mu, mu)
    with pytest.raises(VargpHipError):
        ops.softmax_site_noise(0, 2, 3, 5, device='cpu')
    with pytest.raises(VargpHipError):
        sites.composed_softmax_sites(mu, mu, torch.zeros(5, dtype=torch.int64), None, torch.zeros(2, 3, 5))
