"""The differentiable site bound (vargp_amd/sites.py: site_bound, fit_sites_; ops.site_bound_diff on the fused backward
csrc/sites.hip: vargp_site_bound_bwd), the part that needs no GPU: an fp64 restatement of the bound at a FIXED whitened q(v_t) as a
differentiable torch function on top of tests/test_sites_host.py's and tests/test_collapsed_grad.py's pieces -- the yardstick of
tests/test_hip_site_bound.py -- pinned against ref_newton's value and against central differences; the envelope property that makes
the M-step's partial gradient the gradient of the re-converged bound; the C-ABI entry's symbols, argument checks and workspace
bound; and what the Python surface refuses."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from test_collapsed import _Data, make_problem
from test_collapsed_grad import _MaternOfR2, ref_whiten_diff
from test_sites_host import F64, _kl, _mv, make_targets, ref_ell, ref_newton, ref_sites

DF = 4.0


# -- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_cross(theta, Z, X, nu2):
    """K(Z, X) (G, Mt, N) fp64 that autograd can differentiate at coincident points (test_collapsed_grad._MaternOfR2)."""
    r2 = (((Z.unsqueeze(-2) - X.unsqueeze(0).unsqueeze(-3)) / theta[:-1].exp()) ** 2).sum(-1)
    return (2.0 * theta[-1]).exp() * ((-0.5 * r2).exp() if nu2 == 0 else _MaternOfR2.apply(r2, nu2))


def ref_data_term(kind, par, theta, Z, X, alpha, Q, y, w, nu2):
    """sum_n w_n E_{N(mu_n, var_n)} log p(y_n | f) (G,) fp64 -- ref_sites' sums[:, 0] -- differentiable in theta, Z, alpha, Q and
    par['log_scale'].  Q enters through its symmetric part; the variance clamp passes no gradient (clamp_min), and where it binds
    the quadrature is evaluated at var = 0 as a constant (sqrt has no derivative there)."""
    theta, Z, X, alpha, Q, y = (t.to(F64) for t in (theta, Z, X, alpha, Q, y))
    K = ref_cross(theta, Z, X, nu2)
    y = y.expand(K.shape[0], -1)
    mu = (alpha.unsqueeze(-1) * K).sum(-2)
    raw = (2.0 * theta[-1]).exp() - (K * ((0.5 * (Q + Q.mT)) @ K)).sum(-2)
    pos = raw > 0
    ell = torch.where(pos, ref_ell(kind, par, mu, torch.where(pos, raw, torch.ones_like(raw)), y),
                      ref_ell(kind, par, mu, torch.zeros_like(raw), y))
    if w is None:
        return ell.sum(-1)
    w = w.to(F64)
    return torch.where(w != 0, w * ell, torch.zeros_like(ell)).sum(-1)


def ref_alpha_q(theta, z_all, prev, nu2, a_t, H_t):
    """alpha = T^T a (C, Mt) and Q = T^T (I - H H^T) T (C, Mt, Mt), differentiable in theta and z_all; (a_t, H_t) constants."""
    L, T, a_lt, H = ref_whiten_diff(theta, z_all, prev, nu2)
    C, Mt = z_all.shape[:2]
    a = torch.cat([a_lt, a_t.to(F64)], -1)
    Hb = torch.stack([torch.block_diag(*[Hi[c] for Hi in H], H_t[c].to(F64)) for c in range(C)])
    Q = T.mT @ (torch.eye(Mt, dtype=F64) - Hb @ Hb.mT) @ T
    return _mv(T.mT, a), 0.5 * (Q + Q.mT), L, T


def ref_site_bound(kind, par, theta, z_lt, z_t, prev, x, y, w, nu2, a_t, H_t):
    """The bound (C,) at the FIXED whitened q(v_t) = N(a_t, H_t H_t^T): differentiable in theta, z_t and par['log_scale']; the
    frozen tasks' z_lt, u_mean, u_tril are constants, their whitened moments depend on theta and z through T."""
    z_all = torch.cat([z_lt.to(F64), z_t.to(F64)], -2)
    alpha, Q, _, _ = ref_alpha_q(theta.to(F64), z_all, prev, nu2, a_t, H_t)
    H64 = H_t.to(F64)
    return ref_data_term(kind, par, theta, z_all, x, alpha, Q, y, w, nu2) - _kl(a_t.to(F64), H64 @ H64.mT)


def _problem(kind, t, seed, M=6, N=40, D=2, C=2):
    pr = make_problem(C, M, t, D, N, seed=seed, weights=True)
    y = make_targets(kind, pr, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    a_t = 0.3 * torch.randn(C, M, generator=g, dtype=F64)
    H_t = (0.2 * torch.randn(C, M, M, generator=g, dtype=F64)).tril(-1) + 0.7 * torch.eye(M, dtype=F64)
    par = dict(log_scale=torch.tensor([-0.6, -0.3], dtype=F64), df=DF) if kind == 'studentt' else {}
    # the frozen tasks' q(u) as a fitted model holds it: modest in WHITENED coordinates.  (make_problem's random u_mean is O(1) in
    # the space of u; through T, whose norm reaches jitter^-1/2 for 18 RBF points in the plane, it becomes a latent mean of 1e3
    # and more, where exp and the probit tail leave nothing for a central difference to resolve.)
    L = ref_whiten_diff(pr['theta'].double(), pr['z_all'].double(), [], 0)[0]
    for i, p in enumerate(pr['prev']):
        L_ii = L[:, i * M:(i + 1) * M, i * M:(i + 1) * M]
        a_i = 0.3 * torch.randn(C, M, 1, generator=g, dtype=F64)
        H_i = (0.2 * torch.randn(C, M, M, generator=g, dtype=F64)).tril(-1) + 0.7 * torch.eye(M, dtype=F64)
        pr['prev'][i] = dict(p, u_mean=L_ii @ a_i, u_tril=L_ii @ H_i)
    return pr, y, a_t, H_t, par


def _central(f, base, k, h):
    fd = torch.zeros_like(base[k])
    for e in range(base[k].numel()):
        hi, lo = [q.clone() for q in base], [q.clone() for q in base]
        hi[k].view(-1)[e] += h
        lo[k].view(-1)[e] -= h
        fd.view(-1)[e] = (f(*hi) - f(*lo)) / (2.0 * h)
    return fd


@pytest.mark.parametrize('nu2', [0, 3])
@pytest.mark.parametrize('t', [0, 2])
@pytest.mark.parametrize('kind', ['probit', 'poisson', 'studentt'])
def test_restated_bound_is_ref_newtons_and_its_gradient_is_the_central_difference(kind, t, nu2):
    """M = 6, D = 2, N = 40, two outputs, weights, fp64: the value is ref_newton's bound at the same q (its trace[0]) to 1e-10, the
    data term is ref_sites' sums[:, 0]; every entry of autograd's gradient for (theta, z_t, log_scale) is the central difference
    (h = 1e-5: truncation ~ h^2, rounding ~ 1e-16 |bound| / h) to 1e-6 of the gradient's largest entry -- the step and tolerance of
    tests/test_collapsed_grad.py's central-difference test."""
    M = 6
    pr, y, a_t, H_t, par = _problem(kind, t, seed=50 + t)
    z_lt, z_t = pr['z_all'][:, :t * M].double(), pr['z_all'][:, t * M:].double()
    theta = pr['theta'].double()
    alpha, Q, L, T = ref_alpha_q(theta, pr['z_all'].double(), pr['prev'], nu2, a_t, H_t)
    L_tt = L[:, t * M:, t * M:]
    newton = ref_newton(kind, par, theta, pr['z_all'], pr['prev'], pr['x'], y, pr['w'], nu2, _mv(L_tt, a_t).unsqueeze(-1),
                        L_tt @ H_t, n_iters=0)
    ls = par['log_scale'] if kind == 'studentt' else torch.zeros(2, dtype=F64)

    def bound(th, zt, s):
        p = dict(log_scale=s, df=DF) if kind == 'studentt' else {}
        return ref_site_bound(kind, p, th, z_lt, zt, pr['prev'], pr['x'], y, pr['w'], nu2, a_t, H_t)

    leaves = [q.clone().requires_grad_(True) for q in (theta, z_t, ls)]
    val = bound(*leaves)
    assert torch.allclose(val.detach(), newton['trace'][0], rtol=1e-10, atol=0.0)
    sites = ref_sites(kind, par, theta, pr['z_all'], pr['x'], alpha, Q, y, pr['w'], nu2)
    data = ref_data_term(kind, par, theta, pr['z_all'].double(), pr['x'], alpha, Q, y, pr['w'], nu2)
    assert torch.allclose(data, sites['sums'][:, 0], rtol=1e-12, atol=0.0)
    grads = torch.autograd.grad(val.sum(), leaves, allow_unused=True)
    f = lambda *a: bound(*a).sum().item()
    for k in range(3 if kind == 'studentt' else 2):
        fd = _central(f, [theta, z_t, ls], k, 1e-5)
        err = (fd - grads[k]).abs().max().item() / grads[k].abs().max().item()
        print(f'{kind} t={t} nu2={nu2} parameter {k}: |grad| {grads[k].abs().max().item():.3e}, central-difference mismatch {err:.2e}')
        assert err < 1e-6, (kind, t, nu2, k, err)


@pytest.mark.parametrize('kind', ['probit', 'poisson'])
def test_envelope_partial_gradient_is_the_gradient_of_the_reconverged_bound(kind):
    """At a q that ref_newton has converged tightly (tol 1e-14; log-concave likelihoods) the PARTIAL gradient of the bound for
    (theta, z_t) at the fixed whitened q equals the central difference of the bound RE-CONVERGED at the moved parameters (the
    envelope theorem: d bound / d q = 0 there).  The mismatch (max-abs over the entries, relative to the gradient's largest) is
    printed at h = 1e-3 and h / 2 (both in the truncation regime: each figure falls by 4 from h to h / 2) and asserted against 4 x the figure the restatement's own fixed-q central difference gives at
    h / 2 on the same problem -- no number chosen in advance.
    Printed by this test:
      probit : envelope 7.6e-07 (h) 1.9e-07 (h/2), fixed-q 1.6e-06 (h) 3.9e-07 (h/2)
      poisson: envelope 6.4e-07 (h) 1.4e-07 (h/2), fixed-q 8.4e-06 (h) 2.1e-06 (h/2)"""
    M, nu2, t = 6, 0, 0
    pr, y, a0, H0, par = _problem(kind, t, seed=70)
    theta, z_t = pr['theta'].double(), pr['z_all'].double()
    z_lt = z_t[:, :0]

    def converge(th, zt):
        _, _, L, _ = ref_alpha_q(th, zt, [], nu2, a0, H0)
        return ref_newton(kind, par, th, zt, [], pr['x'], y, pr['w'], nu2, _mv(L, a0).unsqueeze(-1), L @ H0, n_iters=60, tol=1e-14)

    fit = converge(theta, z_t)
    assert fit['n_iters'] < 60
    a_t, H_t = fit['a_t'], torch.linalg.cholesky(fit['Sigma_t'])
    fixed = lambda th, zt: ref_site_bound(kind, par, th, z_lt, zt, [], pr['x'], y, pr['w'], nu2, a_t, H_t)
    leaves = [q.clone().requires_grad_(True) for q in (theta, z_t)]
    grads = torch.autograd.grad(fixed(*leaves).sum(), leaves)
    scale = max(g.abs().max().item() for g in grads)
    f_fixed = lambda th, zt: fixed(th, zt).sum().item()
    f_conv = lambda th, zt: converge(th, zt)['trace'][-1].sum().item()
    h = 1e-3
    env, own = {}, {}
    for step in (h, 0.5 * h):
        env[step] = max((_central(f_conv, [theta, z_t], k, step) - grads[k]).abs().max().item() for k in range(2)) / scale
        own[step] = max((_central(f_fixed, [theta, z_t], k, step) - grads[k]).abs().max().item() for k in range(2)) / scale
    print(f'{kind}: envelope {env[h]:.1e} (h) {env[0.5 * h]:.1e} (h/2), fixed-q {own[h]:.1e} (h) {own[0.5 * h]:.1e} (h/2)')
    assert env[0.5 * h] <= 4.0 * own[0.5 * h], (kind, env, own)


# -- the C ABI ----------------------------------------------------------------------------------------------------------------------
BWD_SYMBOLS = ('vargp_site_bound_bwd', 'vargp_site_bound_bwd_workspace_bytes', 'vargp_site_bound_bwd_chunks')


def test_new_symbols_are_exported_and_declared():
    from vargp_amd import _lib, ops
    text = open(os.path.join(ROOT, 'include', 'vargp_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in BWD_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
        assert re.search(r'\b%s\s*\(' % name, text), f'{name} is not declared in include/vargp_hip.h'
    L = _lib.lib()
    assert L.vargp_site_bound_bwd.restype is ctypes.c_int and len(L.vargp_site_bound_bwd.argtypes) == 26
    assert L.vargp_site_bound_bwd_workspace_bytes.restype is ctypes.c_size_t
    assert L.vargp_site_bound_bwd_chunks(3, 65, 513, 33) >= 2 and L.vargp_site_bound_bwd_chunks(3, 65, 256, 33) == 1
    assert ops.site_bound_bwd_chunks(3, 65, 513, 33) == L.vargp_site_bound_bwd_chunks(3, 65, 513, 33)
    assert callable(ops.site_bound_bwd) and callable(ops.site_bound_diff)


def test_cabi_argument_errors_before_any_launch():
    """A null pointer other than w (and log_scale / gls unless Student-t), a size < 1, Mt above the LDS limit, G > 65535, an unknown
    kind or nu2, a bad ldy or df, a short or misaligned workspace: VARGP_EINVAL (-1) with host memory for pointers -- nothing is
    launched, so no device is touched."""
    from vargp_amd._lib import lib
    L = lib()
    EINVAL = -1
    G, Mt, N, D = 2, 5, 9, 3
    need = L.vargp_site_bound_bwd_workspace_bytes(G, Mt, N, D)
    buf = (ctypes.c_double * (need // 8 + 16))()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)

    def call(ptrs=None, ldy=N, w=p, kind=0, log_scale=p, df=4.0, outs=None, dims=(G, Mt, N, D), nu2=0, ws=p, ws_bytes=need):
        ptrs, outs = ptrs or [p] * 6, outs or [p] * 6                      # outs: gout, gZ, gtheta, galpha, gv, gls
        return L.vargp_site_bound_bwd(*ptrs, ldy, w, kind, log_scale, df, 0.0, *outs, *dims, nu2, ws, ws_bytes, None)

    for bad in range(6):
        assert call(ptrs=[null if q == bad else p for q in range(6)]) == EINVAL
    for bad in range(5):
        assert call(outs=[null if q == bad else p for q in range(6)]) == EINVAL
    assert call(kind=3, outs=[p] * 5 + [null]) == EINVAL and call(kind=3, log_scale=null) == EINVAL
    assert call(kind=3, df=0.0) == EINVAL and call(kind=3, df=-1.0) == EINVAL
    assert call(ws=null) == EINVAL
    for dims in ((0, Mt, N, D), (G, 0, N, D), (G, Mt, 0, D), (G, Mt, N, 0), (-1, Mt, N, D), (65536, Mt, N, D), (G, 257, N, D)):
        assert call(dims=dims, ws_bytes=1 << 40) == EINVAL, dims
    for kind in (-1, 4):
        assert call(kind=kind) == EINVAL
    for nu2 in (-1, 2, 4, 6):
        assert call(nu2=nu2) == EINVAL
    assert call(ldy=N - 1) == EINVAL and call(ldy=-1) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and call(ws_bytes=0) == EINVAL
    assert call(ws=ctypes.c_void_p(ctypes.addressof(buf) + 4), ws_bytes=need) == EINVAL          # misaligned
    assert b'site_bound_bwd' in L.vargp_last_error()


def test_workspace_does_not_grow_with_the_data():
    """Per-chunk partials only: once the chunk count is maximal for the shape (the workgroup target or the byte budget of the
    partials of P binds) N = 1e4 and N = 1e7 need the same bytes; the chunk count obeys the forward's rule."""
    from vargp_amd._lib import lib
    ws, chunks = lib().vargp_site_bound_bwd_workspace_bytes, lib().vargp_site_bound_bwd_chunks
    for G, Mt, D in ((64, 200, 8), (600, 100, 2), (16, 256, 784), (1024, 15, 40)):
        assert chunks(G, Mt, 10 ** 4, D) == chunks(G, Mt, 10 ** 7, D), (G, Mt, D)
        assert ws(G, Mt, 10 ** 4, D) == ws(G, Mt, 10 ** 7, D) > 0, (G, Mt, D)
    for G, Mt, D in ((1, 100, 8), (10, 200, 784), (3, 256, 33), (1, 15, 2)):
        nt = (Mt + 63) // 64
        for N in (1, 1000, 10 ** 6, 2 * 10 ** 9):
            n = chunks(G, Mt, N, D)
            assert 1 <= n <= min(1024, (N + 255) // 256)
            assert n == 1 or n * G * nt * 64 * (D + 2) * 4 <= 64 << 20
            assert ws(G, Mt, N, D) <= n * G * (nt * 64 * (D + 2) * 4 + D * 4 + 16) + 5 * 256 + 256
        big = [ws(G, Mt, N, D) for N in (10 ** 7, 10 ** 8, 2 * 10 ** 9)]
        assert max(big) <= 1.02 * min(big)                            # (the chunk length is rounded to 64 columns: not exactly equal)
    assert ws(0, 5, 5, 5) == 0 and chunks(1, 0, 5, 5) == 0


# -- the Python surface -------------------------------------------------------------------------------------------------------------
def test_site_bound_and_fit_sites_name_what_they_refuse():
    from vargp_amd._lib import VargpHipError
    from vargp_amd.kernels import DeepRBFKernel
    from vargp_amd.likelihoods import BernoulliLikelihood
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    labels = torch.arange(40) % 3
    reg = _Data(x, x[:, 0].clone())
    counts = _Data(x, torch.arange(40).float() % 4)
    deep = VARGP(torch.randn(1, 4, 3, generator=g), DeepRBFKernel(3, feature_size=6), BernoulliLikelihood())
    bern = VARGP.create_clf(_Data(x, labels), M=4, likelihood='bernoulli')
    for call in (lambda gp, *a: gp.site_bound(*a), lambda gp, *a: gp.fit_sites_(*a, n_rounds=1, m_steps=1)):
        with pytest.raises(ValueError, match='couples the outputs'):
            call(VARGP.create_clf(_Data(x, labels), M=4), x, labels)
        with pytest.raises(ValueError, match='fit_q_'):
            call(VARGP.create_reg(reg, M=4), x, reg.targets)
        with pytest.raises(ValueError, match='ep_var_mean=True'):
            call(VARGP.create_reg(counts, M=4, likelihood='poisson', ep_var_mean=False), x, counts.targets)
        with pytest.raises(ValueError, match='DeepRBFKernel'):
            call(deep, x, (labels == 0).float())
        with pytest.raises(VargpHipError):                          # a supported model on the host: no CPU path
            call(bern, x, labels)
    for params in ((), ('z', 'q'), ('noise',)):
        with pytest.raises(ValueError, match='params'):
            bern.fit_sites_(x, labels, params=params)
    with pytest.raises(ValueError, match="'lik'"):
        bern.fit_sites_(x, labels, params=('z', 'lik'))
    with pytest.raises(ValueError, match='damping'):
        bern.fit_sites_(x, labels, damping=0.0)
    with pytest.raises(ValueError, match='bernoulli'):
        VARGP.create_clf(_Data(x, labels), M=4, q_init='em')                         # softmax
    with pytest.raises(ValueError, match="'optimal'"):
        VARGP.create_reg(reg, M=4, q_init='em')                                      # gaussian


def test_site_bound_diff_refuses_what_it_cannot_differentiate():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    theta, Z, X, y = torch.zeros(4), torch.randn(1, 5, 3), torch.randn(9, 3), torch.rand(1, 9).round()
    alpha, Q = torch.zeros(1, 5), torch.zeros(1, 5, 5)
    for name, kw in (('X', dict(X=X.clone().requires_grad_(True))), ('y', dict(y=y.clone().requires_grad_(True))),
                     ('w', dict(w=torch.rand(1, 9).requires_grad_(True)))):
        args = dict(theta=theta, Z=Z, X=X, alpha=alpha, Q=Q, y=y, w=None, kind='bernoulli', extra=(0,))
        args.update(kw)
        with pytest.raises(ValueError, match=f'{name} requires grad'):
            ops.site_bound_diff(**args)
    with pytest.raises(VargpHipError):
        ops.site_bound_diff(theta.requires_grad_(True), Z, X, alpha, Q, y, None, 'bernoulli', (0,))


def test_whitened_q_helpers_exist():
    from vargp_amd import sites
    assert callable(sites.whitened_q) and callable(sites.set_whitened_q_) and sites.EMFit._fields == ('bound', 'n_rounds', 'n_newton', 'stopped')
