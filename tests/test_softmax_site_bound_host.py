"""The differentiable softmax site bound (vargp_amd/sites.py: softmax_site_bound, fit_softmax_sites_; ops.softmax_site_bound_diff on
csrc/softmax_sites.hip: vargp_softmax_site_grads and csrc/sites.hip: vargp_site_transport_bwd), the part that needs no GPU: an fp64
restatement of fit_q_softmax_'s bound at a FIXED whitened q(v_t) and FIXED noise as a differentiable torch function -- the
yardstick of tests/test_hip_softmax_site_bound.py -- pinned against ref_softmax_newton's value and against torch.autograd.gradcheck;
one EM round of the restatement, whose gain is the margin the device test relies on; the C-ABI entries' symbols and argument
checks; and what the Python surface refuses."""
import ctypes
import importlib.util
import math
import os
import re

import pytest
import torch

from conftest import ROOT
from test_collapsed import _Data, ref_kernel, ref_whiten
from test_site_bound_host import ref_alpha_q, ref_cross
from test_sites_host import _kl, _mv
from test_softmax_sites_host import blobs, ref_softmax_newton

F64 = torch.float64


# -- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_softmax_marginals(theta, Z, X, alpha, Q, nu2):
    """mu = alpha . k_n and the UNCLAMPED gamma^2 - k_n^T Qs k_n (C, N) fp64, differentiable in theta, Z, alpha and Q (through its
    symmetric part); K from test_site_bound_host.ref_cross, which autograd can differentiate at coincident points."""
    theta, Z, X, alpha, Q = (t.to(F64) for t in (theta, Z, X, alpha, Q))
    K = ref_cross(theta, Z, X, nu2)
    mu = (alpha.unsqueeze(-1) * K).sum(-2)
    return mu, (2.0 * theta[-1]).exp() - (K * ((0.5 * (Q + Q.mT)) @ K)).sum(-2)


def ref_softmax_value(mu, raw, y, w, eps):
    """sum_n w_n [mu_{y_n, n} - mean_f logsumexp(mu_n + sqrt(var_n) o eps_nf)] (1,) fp64 with var = max(raw, 0): the clamp passes no
    gradient, and where it binds the draw is evaluated at var = 0 as a constant (sqrt has no derivative there)."""
    pos = raw > 0
    sd = torch.where(pos, torch.where(pos, raw, torch.ones_like(raw)).sqrt(), torch.zeros_like(raw))
    lse = torch.logsumexp(mu + sd * eps.to(F64), -2).mean(0)
    ell = mu[y, torch.arange(mu.shape[-1])] - lse
    if w is None:
        return ell.sum().view(1)
    w = w.to(F64)
    return torch.where(w != 0, w * ell, torch.zeros_like(ell)).sum().view(1)


def ref_softmax_data_term(theta, Z, X, alpha, Q, y, w, eps, nu2):
    """ref_softmax_sites' sums[0] at the marginals of (alpha, Q), (1,) fp64, differentiable in theta, Z, alpha and Q."""
    return ref_softmax_value(*ref_softmax_marginals(theta, Z, X, alpha, Q, nu2), y, w, eps)


def ref_softmax_site_bound(theta, z_lt, z_t, prev, x, y, w, nu2, a_t, H_t, eps):
    """fit_q_softmax_'s bound (1,) at the FIXED whitened q(v_t) = N(a_t, H_t H_t^T) and the FIXED noise eps (F, C, N):
    differentiable in theta and z_t; the frozen tasks' z_lt, u_mean, u_tril are constants, their whitened moments depend on theta
    and z through T."""
    z_all = torch.cat([z_lt.to(F64), z_t.to(F64)], -2)
    alpha, Q, _, _ = ref_alpha_q(theta.to(F64), z_all, prev, nu2, a_t, H_t)
    H64 = H_t.to(F64)
    return ref_softmax_data_term(theta, z_all, x, alpha, Q, y, w, eps, nu2) - _kl(a_t.to(F64), H64 @ H64.mT).sum().view(1)


def _random_q(C, M, g):
    a_t = 0.3 * torch.randn(C, M, generator=g, dtype=F64)
    return a_t, (0.2 * torch.randn(C, M, M, generator=g, dtype=F64)).tril(-1) + 0.7 * torch.eye(M, dtype=F64)


@pytest.mark.parametrize('nu2', [0, 3])
@pytest.mark.parametrize('t', [0, 1])
def test_restated_value_is_ref_softmax_newtons_at_iteration_0(t, nu2):
    """C = 3, M = 6, N = 40, F = 4, weights with zeros, with and without a frozen task: the restatement at the whitened q of
    (u_mean, u_tril) equals the bound ref_softmax_newton reports before its first step, to 1e-12 relative."""
    C, M, N, D, F = 3, 6, 40, 2, 4
    g = torch.Generator().manual_seed(60 + t)
    x, y = blobs(C, N, D, 60 + t)
    z_all = torch.stack([x[torch.randperm(N, generator=g)[:M * (t + 1)]] for _ in range(C)])
    theta = torch.cat([torch.full((D,), math.log(1.5)), torch.tensor([0.1])]).double()
    L = ref_whiten(theta, z_all, [], nu2)[0]
    prev = []
    if t:
        a_0, H_0 = _random_q(C, M, g)
        prev = [dict(u_mean=L[:, :M, :M] @ a_0.unsqueeze(-1), u_tril=L[:, :M, :M] @ H_0)]
    a_t, H_t = _random_q(C, M, g)
    L_tt = L[:, t * M:, t * M:]
    w = torch.rand(N, generator=g) + 0.25
    w[::7] = 0.0
    eps = torch.randn(F, C, N, generator=g, dtype=F64)
    newton = ref_softmax_newton(theta, z_all, prev, x, y, w, nu2, _mv(L_tt, a_t).unsqueeze(-1), L_tt @ H_t, eps, n_iters=0)
    val = ref_softmax_site_bound(theta, z_all[:, :t * M], z_all[:, t * M:], prev, x, y, w, nu2, a_t, H_t, eps)
    assert tuple(val.shape) == (1,) and torch.allclose(val, newton['trace'][0], rtol=1e-12, atol=0.0)
    # ... and ref_kernel's cross-kernel is ref_cross' away from coincident points
    assert torch.allclose(ref_cross(theta, z_all.double(), x.double() + 0.5, nu2),
                          ref_kernel(z_all.double(), (x.double() + 0.5).unsqueeze(0), theta, nu2), rtol=1e-12, atol=1e-300)


def test_gradcheck_of_the_restatement():
    """torch.autograd.gradcheck in fp64 at C = 3, Mt = 5, N = 7, F = 2 for theta, Z, alpha and Q, with no variance at the clamp
    (the smallest is asserted to be above 0.05 gamma^2): the restatement's autograd IS the derivative of the sampled value."""
    C, Mt, N, D, F = 3, 5, 7, 2, 2
    g = torch.Generator().manual_seed(5)
    X = torch.randn(N, D, generator=g, dtype=F64)
    Z = torch.randn(C, Mt, D, generator=g, dtype=F64)
    theta = torch.cat([math.log(1.2) + 0.1 * torch.randn(D, generator=g, dtype=F64), torch.tensor([math.log(0.9)], dtype=F64)])
    alpha = 0.5 * torch.randn(C, Mt, generator=g, dtype=F64)
    R = torch.randn(C, Mt, Mt, generator=g, dtype=F64)
    Q = 0.02 * (R @ R.mT) + 0.01 * torch.randn(C, Mt, Mt, generator=g, dtype=F64)          # (not symmetric: through its symmetric part)
    y = torch.arange(N) % C
    w = torch.rand(N, generator=g, dtype=F64) + 0.25
    eps = torch.randn(F, C, N, generator=g, dtype=F64)
    raw = ref_softmax_marginals(theta, Z, X, alpha, Q, 0)[1]
    assert raw.min().item() > 0.05 * math.exp(2.0 * theta[-1].item())
    for nu2 in (0, 5):
        f = lambda th, z, al, q: ref_softmax_data_term(th, z, X, al, q, y, w, eps, nu2)
        leaves = [t.clone().requires_grad_(True) for t in (theta, Z, alpha, Q)]
        assert torch.autograd.gradcheck(f, leaves, eps=1e-6, atol=1e-7, rtol=1e-5)


def test_variance_of_zero_passes_no_gradient():
    """Q scaled until some, not all, variances clamp: the value and every gradient stay finite (autograd's chain through sqrt at
    0 would be inf x 0 = NaN), and sites.softmax_value_torch, the composed route's fp32 form, agrees on the value and on the
    derivatives for (mu, var), exact zeros at the clamp included."""
    C, Mt, N, D, F = 2, 4, 6, 2, 3
    g = torch.Generator().manual_seed(7)
    X, Z = torch.randn(N, D, generator=g, dtype=F64), torch.randn(C, Mt, D, generator=g, dtype=F64)
    theta = torch.zeros(D + 1, dtype=F64)
    alpha = torch.randn(C, Mt, generator=g, dtype=F64)
    R = torch.randn(C, Mt, Mt, generator=g, dtype=F64)
    Q = 1.5 * (R @ R.mT)
    raw = ref_softmax_marginals(theta, Z, X, alpha, Q, 0)[1]
    assert 0 < int((raw <= 0).sum()) < raw.numel()
    eps = torch.randn(F, C, N, generator=g, dtype=F64)
    leaves = [t.clone().requires_grad_(True) for t in (theta, Z, alpha, Q)]
    val = ref_softmax_data_term(*leaves[:2], X, *leaves[2:], torch.arange(N) % C, None, eps, 0)
    grads = torch.autograd.grad(val.sum(), leaves)
    assert bool(torch.isfinite(val).all()) and all(bool(torch.isfinite(t).all()) for t in grads)
    from vargp_amd import sites
    mu, raw = ref_softmax_marginals(theta, Z, X, alpha, Q, 0)
    y = torch.arange(N) % C
    a = [mu.clone().requires_grad_(True), raw.clamp_min(0.0).requires_grad_(True)]
    b = [mu.float().requires_grad_(True), raw.clamp_min(0.0).float().requires_grad_(True)]
    va, vb = ref_softmax_value(*a, y, None, eps), sites.softmax_value_torch(*b, y, None, eps.float())
    ga, gb = torch.autograd.grad(va.sum(), a), torch.autograd.grad(vb, b)
    assert vb.item() == pytest.approx(va.item(), rel=1e-5)
    for u, v in zip(ga, gb):
        assert torch.allclose(u, v.double(), rtol=1e-4, atol=1e-5)
    assert bool((ga[1][raw <= 0] == 0).all()) and bool((gb[1][raw <= 0] == 0).all())


# -- one EM round of the restatement ----------------------------------------------------------------------------------------------
EM_C, EM_M, EM_D, EM_N, EM_F = 3, 10, 2, 300, 32
EM_SEED = 41                     # the data seed: chosen so that the round below gains >= EM_MARGIN |bound| in the restatement alone
EM_LENGTHSCALE = 1.5
EM_MARGIN = 1e-3
EM_STEP = 1e-2                   # a plain-gradient M-step moves every parameter by at most this (the scale of a Yogi step of lr 1e-2)


def em_inputs(kernel='rbf', seed=EM_SEED, M=EM_M, prev=None, turn=0.0):
    """The model-level problem both files use: three blobs, M inducing points per class at random data points, lengthscales 1.5.
    -> (gp on the host, x, y)"""
    from vargp_amd.kernels import MaternKernel, RBFKernel
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.vargp import VARGP
    x, y = blobs(EM_C, EM_N, EM_D, seed, turn=turn)
    g = torch.Generator().manual_seed(seed + 1000)
    z = torch.stack([x[torch.randperm(EM_N, generator=g)[:M]] for _ in range(EM_C)])
    torch.manual_seed(seed)
    kern = RBFKernel(EM_D, map_est=True) if kernel == 'rbf' else MaternKernel(EM_D, nu=1.5, map_est=True)
    with torch.no_grad():
        kern.log_mean[:EM_D] = math.log(EM_LENGTHSCALE)
    return VARGP(z, kern, MulticlassSoftmax(n_f=10), n_var_samples=1, prev_params=[dict(p) for p in (prev or [])]), x, y


def test_one_em_round_of_the_restatement_raises_the_bound():
    """E-step: ref_softmax_newton from the prior to its end; M-step: 5 plain-gradient steps on (theta, z) at the fixed whitened
    q, each scaled so that no parameter moves by more than EM_STEP.  The bound at the fixed q rises by at least EM_MARGIN |bound|:
    far above the fp32 error of the device's bound (1e-5 relative, tests/test_hip_softmax_sites.py), so the device's first round
    is decided by the same margin."""
    gp, x, y = em_inputs()
    g = torch.Generator().manual_seed(EM_SEED + 2000)
    eps = torch.randn(EM_F, EM_C, EM_N, generator=g, dtype=F64)
    theta, z = gp.kernel.log_mean.detach().double(), gp.z.detach().double()
    L = ref_whiten(theta, z, [], 0)[0]
    fit = ref_softmax_newton(theta, z, [], x, y, None, 0, torch.zeros(EM_C, EM_M, 1), L, eps)
    a_t, H_t = fit['a_t'], torch.linalg.cholesky(fit['Sigma_t'])
    bound = lambda th, zt: ref_softmax_site_bound(th, zt[:, :0], zt, [], x, y, None, 0, a_t, H_t, eps)
    before = bound(theta, z).item()
    assert before == pytest.approx(fit['trace'][-1].item(), rel=1e-9)
    for _ in range(5):
        leaves = [theta.clone().requires_grad_(True), z.clone().requires_grad_(True)]
        grads = torch.autograd.grad(bound(*leaves).sum(), leaves)
        scale = EM_STEP / max(t.abs().max().item() for t in grads)
        theta, z = theta + scale * grads[0], z + scale * grads[1]
    after = bound(theta, z).item()
    print(f'E-step {fit["n_iters"]} iterations, bound {before:.4f}; after the M-step {after:.4f}: gain {(after - before) / abs(before):.3e}')
    assert after - before >= EM_MARGIN * abs(before)


# -- the C ABI ----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('vargp_softmax_site_grads', 'vargp_site_transport_bwd', 'vargp_site_transport_bwd_workspace_bytes',
               'vargp_site_transport_bwd_chunks')
EINVAL = -1


def test_new_symbols_are_exported_and_declared():
    from vargp_amd import _lib, ops
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vargp_hip.h')).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
        assert re.search(r'\b%s\s*\(' % name, text), f'{name} is not declared in include/vargp_hip.h'
    L = _lib.lib()
    assert len(L.vargp_softmax_site_grads.argtypes) == 13 and len(L.vargp_site_transport_bwd.argtypes) == 19
    for shape in ((3, 65, 513, 33), (3, 65, 256, 33), (3, 130, 513, 40), (1, 1, 1, 1)):
        assert L.vargp_site_transport_bwd_chunks(*shape) == L.vargp_site_bound_bwd_chunks(*shape)
        assert L.vargp_site_transport_bwd_workspace_bytes(*shape) == L.vargp_site_bound_bwd_workspace_bytes(*shape) > 0
    assert L.vargp_site_transport_bwd_chunks(3, 130, 513, 40) >= 2
    assert L.vargp_site_transport_bwd_chunks(0, 5, 5, 5) == 0 and L.vargp_site_transport_bwd_workspace_bytes(1, 0, 5, 5) == 0
    assert all(callable(f) for f in (ops.softmax_site_grads, ops.site_transport_bwd, ops.site_transport_bwd_chunks,
                                     ops.softmax_site_bound_diff))


def test_softmax_site_grads_argument_errors_before_any_launch():
    from vargp_amd._lib import lib
    L = lib()
    C, N, F = 3, 9, 2
    buf = (ctypes.c_double * 64)()
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)

    def call(mu=p, var=p, y=p, w=p, eps=p, gout=p, gmu=p, gvar=p, dims=(C, N, F)):
        return L.vargp_softmax_site_grads(mu, var, y, w, eps, 0, gout, gmu, gvar, *dims, None)

    for name in ('mu', 'var', 'y', 'gout', 'gmu', 'gvar'):                             # (w and eps are optional)
        assert call(**{name: null}) == EINVAL, name
    for dims in ((1, N, F), (0, N, F), (129, N, F), (C, 0, F), (C, N, 0), (C, N, 65536)):
        assert call(dims=dims) == EINVAL, dims
    assert b'softmax_site_grads' in L.vargp_last_error()
    assert call(dims=(129, N, F)) == EINVAL and b'128' in L.vargp_last_error()


def test_site_transport_bwd_argument_errors_before_any_launch():
    from vargp_amd._lib import lib
    L = lib()
    G, Mt, N, D = 2, 5, 9, 3
    need = L.vargp_site_transport_bwd_workspace_bytes(G, Mt, N, D)
    buf = (ctypes.c_double * (need // 8 + 16))()
    p, null = ctypes.c_void_p(ctypes.addressof(buf)), ctypes.c_void_p(0)

    def call(ptrs=None, dims=(G, Mt, N, D), nu2=0, ws=p, ws_bytes=need):
        return L.vargp_site_transport_bwd(*(ptrs or [p] * 11), *dims, nu2, ws, ws_bytes, None)

    for bad in range(11):
        assert call(ptrs=[null if q == bad else p for q in range(11)]) == EINVAL, bad
    assert call(ws=null) == EINVAL
    for dims in ((0, Mt, N, D), (G, 0, N, D), (G, Mt, 0, D), (G, Mt, N, 0), (-1, Mt, N, D), (65536, Mt, N, D), (G, 257, N, D)):
        assert call(dims=dims, ws_bytes=1 << 40) == EINVAL, dims
    for nu2 in (-1, 2, 4, 6):
        assert call(nu2=nu2) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and call(ws_bytes=0) == EINVAL
    assert call(ws=ctypes.c_void_p(ctypes.addressof(buf) + 4)) == EINVAL              # misaligned
    assert b'site_transport_bwd' in L.vargp_last_error()


# -- the Python surface -------------------------------------------------------------------------------------------------------------
def test_check_softmax_differentiable_names_what_it_refuses():
    from vargp_amd import sites
    from vargp_amd.kernels import DeepRBFKernel, RBFKernel
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    labels = torch.arange(40) % 3
    data = _Data(x, labels)
    with pytest.raises(ValueError, match='MulticlassSoftmax'):
        sites.check_softmax_differentiable(VARGP.create_clf(data, M=4, likelihood='bernoulli'), 'softmax_site_bound')
    deep = VARGP(torch.randn(3, 4, 3, generator=g), DeepRBFKernel(3, feature_size=6), MulticlassSoftmax(n_f=4))
    with pytest.raises(ValueError, match='DeepRBFKernel is not supported .the feature map needs the gradient'):
        sites.check_softmax_differentiable(deep, 'softmax_site_bound')
    sites.check_softmax_supported(deep)                                               # (the fit itself supports it)
    with pytest.raises(ValueError, match='ep_var_mean=True'):
        sites.check_softmax_differentiable(VARGP.create_clf(data, M=4, ep_var_mean=False), 'softmax_site_bound')
    wide = VARGP(torch.randn(129, 2, 3, generator=g), RBFKernel(3), MulticlassSoftmax(n_f=4))
    with pytest.raises(ValueError, match='128'):
        sites.check_softmax_differentiable(wide, 'softmax_site_bound')
    sites.check_softmax_differentiable(VARGP.create_clf(data, M=4), 'softmax_site_bound')
    sites.check_softmax_differentiable(VARGP.create_clf(data, M=4, kernel='matern32'), 'softmax_site_bound')


def test_softmax_site_bound_and_fit_softmax_sites_name_what_they_refuse():
    from vargp_amd._lib import VargpHipError
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    labels = torch.arange(40) % 3
    data = _Data(x, labels)
    gp = VARGP.create_clf(data, M=4)
    bern = VARGP.create_clf(data, M=4, likelihood='bernoulli')
    for call in (lambda m, *a, **k: m.softmax_site_bound(*a, **k), lambda m, *a, **k: m.fit_softmax_sites_(*a, n_rounds=1, m_steps=1, **k)):
        with pytest.raises(ValueError, match='MulticlassSoftmax'):
            call(bern, x, labels)
        with pytest.raises(ValueError, match='n_f'):
            call(gp, x, labels, n_f=0)
        with pytest.raises(ValueError, match='weights'):
            call(gp, x, labels, weights=torch.ones(3, 40))
        with pytest.raises(ValueError, match='int64'):
            call(gp, x, labels.float())
        with pytest.raises(VargpHipError):                          # a supported model on the host: no CPU path
            call(gp, x, labels)
    with pytest.raises(ValueError, match="'lik'"):
        gp.fit_softmax_sites_(x, labels, params=('z', 'lik'))
    for params in ((), ('z', 'q'), ('noise',)):
        with pytest.raises(ValueError, match='params'):
            gp.fit_softmax_sites_(x, labels, params=params)
    with pytest.raises(ValueError, match='damping'):
        gp.fit_softmax_sites_(x, labels, damping=0.0)
    with pytest.raises(ValueError, match='n_rounds'):
        gp.fit_softmax_sites_(x, labels, n_rounds=-1)
    # the independent-output bound and EM still refuse the softmax, with their present messages
    with pytest.raises(ValueError, match='couples the outputs'):
        gp.site_bound(x, labels)
    with pytest.raises(ValueError, match='couples the outputs'):
        gp.fit_sites_(x, labels, n_rounds=1, m_steps=1)


def test_factory_and_driver_know_em_softmax():
    from vargp_amd.vargp import VARGP, _CLF_Q_INITS
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    data = _Data(x, torch.arange(40) % 3)
    assert 'em_softmax' in _CLF_Q_INITS
    with pytest.raises(ValueError, match="'em'"):
        VARGP.create_clf(data, M=4, q_init='em_softmax', likelihood='bernoulli')
    with pytest.raises(ValueError, match='DeepRBFKernel'):
        VARGP.create_clf(data, M=4, q_init='em_softmax', dkl=True)
    with pytest.raises(ValueError, match='bernoulli'):
        VARGP.create_clf(data, M=4, q_init='em')                  # softmax: unchanged
    spec = importlib.util.spec_from_file_location('vargp_driver_for_em_softmax', os.path.join(ROOT, 'experiments', 'vargp.py'))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    args = drv.parse_args(['s_mnist', '--q_init', 'em_softmax', '--em_rounds', '2', '--em_steps', '3', '--site_samples', '8'])
    assert (args.q_init, args.em_rounds, args.em_steps, args.site_samples) == ('em_softmax', 2, 3, 8)


def test_softmax_site_bound_diff_refuses_what_it_cannot_differentiate():
    from vargp_amd import ops, sites
    from vargp_amd._lib import VargpHipError
    theta, Z, X, y = torch.zeros(4), torch.randn(3, 5, 3), torch.randn(9, 3), torch.arange(9) % 3
    alpha, Q = torch.zeros(3, 5), torch.zeros(3, 5, 5)
    for name, kw in (('X', dict(X=X.clone().requires_grad_(True))), ('w', dict(w=torch.rand(9).requires_grad_(True)))):
        args = dict(theta=theta, Z=Z, X=X, alpha=alpha, Q=Q, y=y, w=None, n_f=2)
        args.update(kw)
        with pytest.raises(ValueError, match=f'{name} requires grad'):
            ops.softmax_site_bound_diff(**args)
    for fn in (ops.softmax_site_bound_diff, sites.composed_softmax_site_bound):
        with pytest.raises(VargpHipError):
            fn(theta.clone().requires_grad_(True), Z, X, alpha, Q, y, None, 2)
    mu = torch.zeros(3, 5)
    with pytest.raises(VargpHipError):
        ops.softmax_site_grads(mu, mu, torch.zeros(5, dtype=torch.int64), None, 2, torch.ones(1))
    with pytest.raises(VargpHipError):
        ops.site_transport_bwd(theta, Z, X, alpha, Q, torch.zeros(3, 9), torch.zeros(3, 9))
