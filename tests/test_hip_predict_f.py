"""The full predictive covariance on the device: ops.predictive_cov (csrc/pred_cov.hip), VARGP.predict_f(full_cov=True) and
VARGP.sample_f against the fp64 reference of tests/test_predict_f.py.

Rule (tests/test_hip_random_sweep.py), per case:  err(HIP, fp64) <= RTOL_SCALAR + 2 err(torch fp32 on the host, fp64), with
err = max |a - a_64| / gamma_s^2 for covariances and max |a - a_64| / gamma_s for means and function samples (the natural
scales of the two: gamma_s^2 is the prior variance of hyper-sample s).  The fp32 host evaluation runs on one thread, as in
sweep_rule.py, so that the bound does not depend on the host."""
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import RTOL_SCALAR, to_dev
from test_predict_f import ref_predict_f

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
EPS32 = float(np.finfo(np.float32).eps)
S_OP, C_OP = 2, 3


def _one_thread(fn):
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(n)


def _k_of_d2(d2, nu2):
    d2 = d2.clamp_min(0)
    a = (nu2 * d2).sqrt()
    if nu2 == 1:
        return (-a).exp()
    if nu2 == 3:
        return (1 + a) * (-a).exp()
    return (1 + a + (5.0 / 3.0) * d2) * (-a).exp()


def matern_gram(theta, x, y=None, full_gram=False, nu2=5):
    """Signature of orc.rbf_gram; the Matern kernels restated with the distance formed directly (tests/test_hip_matern.py)."""
    S = theta.shape[0]
    th = theta.reshape(S, *([1] * (x.dim() - 2)), 1, -1)
    sig, g2 = th[..., :-1].exp(), (2.0 * th[..., -1:]).exp()
    a = x.unsqueeze(0) / sig
    b = a if y is None else y.unsqueeze(0) / sig
    return g2 * _k_of_d2(((a.unsqueeze(-2) - b.unsqueeze(-3)) ** 2).sum(-1), nu2)


def _gram(theta, X, nu2):
    """K_theta(X, X) (S, 1, B, B) in the dtype of the inputs: the oracle's RBF, or the Matern restatement above."""
    return orc.rbf_gram(theta, X.unsqueeze(0)) if nu2 == 0 else matern_gram(theta, X.unsqueeze(0), nu2=nu2)


# -- 1, 2. the op -----------------------------------------------------------------------------------------------------------------
def _op_inputs(B, Mt, D, seed, S=S_OP, C=C_OP):
    g = torch.Generator().manual_seed(seed)
    theta = math.log(0.5) + 0.05 * torch.randn(S, D + 1, generator=g)
    X = torch.randn(B, D, generator=g) * math.sqrt(0.25 / D)           # scaled squared distances around 2
    P = 0.5 * torch.randn(S, C, Mt, B, generator=g) / math.sqrt(Mt)    # P^T P and W^T W of the order of K
    W = 0.5 * torch.randn(S, C, Mt, B, generator=g) / math.sqrt(Mt)
    return theta, X, P, W


def _formula(theta, X, P, W, nu2, dtype):
    theta, X, P, W = theta.to(dtype), X.to(dtype), P.to(dtype), W.to(dtype)
    return _gram(theta, X, nu2) - P.mT @ P + W.mT @ W


def _op_case(B, Mt, D, nu2, seed, S=S_OP, C=C_OP):
    """-> (err_hip, err_32, message or None) of one case; also asserts nothing itself."""
    from vargp_amd import ops
    theta, X, P, W = _op_inputs(B, Mt, D, seed, S, C)
    s64 = _formula(theta, X, P, W, nu2, torch.float64)
    s32 = _one_thread(lambda: _formula(theta, X, P, W, nu2, torch.float32))
    td, Xd, Pd, Wd = theta.to(DEV), X.to(DEV), P.to(DEV), W.to(DEV)
    got = ops.predictive_cov(td, Xd, Pd, Wd, nu2)
    assert got.shape == (S, C, B, B) and got.dtype == torch.float32
    g2 = (2.0 * theta[:, -1].double()).exp().view(S, 1, 1, 1)
    e_hip = ((got.cpu().double() - s64).abs() / g2).max().item()
    e_32 = ((s32.double() - s64).abs() / g2).max().item()
    tag = f'B{B} Mt{Mt} D{D} nu2={nu2}'
    msgs = []
    if not e_hip <= RTOL_SCALAR + 2.0 * e_32:
        msgs.append(f'{tag}: err {e_hip:.2e} > {RTOL_SCALAR:.0e} + 2 x {e_32:.2e}')
    # structure: bitwise symmetric; the diagonal is predictive_diag's variance up to the order of 2 Mt + 1 fp32 terms
    if not torch.equal(got, got.mT):
        msgs.append(f'{tag}: not bitwise symmetric')
    kd = (2.0 * td[:, -1]).exp().view(S, 1).expand(S, C).contiguous()
    _, var = ops.predictive_diag(Pd, Wd, torch.zeros(S, C, Mt, device=DEV), kd)
    bound = 2 * (2 * Mt + 1) * EPS32 * (g2.squeeze(-1) + (P.double() ** 2).sum(-2) + (W.double() ** 2).sum(-2))
    gap = (got.diagonal(dim1=-2, dim2=-1).cpu().double() - var.cpu().double()).abs()
    if not bool((gap <= bound).all()):
        msgs.append(f'{tag}: diagonal off predictive_diag by {(gap / bound).max().item():.2f} of the bound')
    return e_hip, e_32, gap.max().item(), msgs


BS, MTS, DS = (1, 31, 32, 33, 65, 100), (1, 20, 33, 130), (2, 32, 33, 40)


@pytest.mark.parametrize('nu2', [0, 1, 3, 5])
def test_op_vs_fp64_and_structure(nu2):
    """Full cross product of the sizes (96 cases per kernel, S x C = 2 x 3): against fp64 by the sweep rule, bitwise symmetry,
    and the diagonal against ops.predictive_diag within 2 (2 Mt + 1) eps (gamma^2 + sum P^2 + sum W^2) per column -- the
    forward-error bound of two fp32 sums of the same 2 Mt + 1 terms in different orders."""
    bad, worst = [], (0.0, None)
    for i, (B, Mt, D) in enumerate(itertools.product(BS, MTS, DS)):
        e_hip, e_32, gap, msgs = _op_case(B, Mt, D, nu2, seed=1000 * nu2 + i)
        bad += msgs
        r = e_hip / (RTOL_SCALAR + 2.0 * e_32)
        if r > worst[0]:
            worst = (r, f'B{B} Mt{Mt} D{D}: err {e_hip:.2e}, fp32 host {e_32:.2e}')
    print(f'nu2={nu2}: worst case {worst[1]} ({worst[0]:.3f} of the bound)')
    assert not bad, bad


@pytest.mark.parametrize('nu2', [0, 5])
@pytest.mark.parametrize('D', [2, 40])
def test_op_large_tile_path(nu2, D):
    """B above 256 takes the 128 x 128 tiles (csrc/pred_cov.hip: kPcSmallB); B = 300 is three tiles per side, the last one
    ragged, with mirrored tiles below the diagonal."""
    e_hip, e_32, gap, msgs = _op_case(300, 33, D, nu2, seed=77 + nu2 + D, S=1, C=2)
    print(f'B300 Mt33 D{D} nu2={nu2}: err {e_hip:.2e}, fp32 host {e_32:.2e}, diagonal gap {gap:.2e}')
    assert not msgs, msgs


def test_op_bad_arguments():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    theta, X, P, W = to_dev(list(_op_inputs(5, 3, 4, 0)), DEV)
    with pytest.raises(VargpHipError):
        ops.predictive_cov(theta, X, P, W, 2)


# -- 3. the model -----------------------------------------------------------------------------------------------------------------
def _fill(gp, params):
    with torch.no_grad():
        gp.kernel.log_mean.copy_(params['log_mean'])
        gp.kernel.log_logvar.copy_(params['log_logvar'])
        gp.u_mean.copy_(params['u_mean'])
        gp.u_tril_vec.copy_(params['u_tril_vec'])
    return gp.to(DEV)


def _model(case):
    """-> (gp, params, prev, x, nz, nu2, phi) of a named case."""
    from vargp_amd.kernels import DeepRBFKernel, MaternKernel, RBFKernel
    from vargp_amd.likelihoods import GaussianLikelihood, MulticlassSoftmax
    from vargp_amd.vargp import VARGP
    S, F_, C = 2, 3, 3
    kind, M, D, B, n_prev, nomean = {
        'rbf-M20-D2-B33': ('rbf', 20, 2, 33, 0, False),
        'rbf-M36-D40-B65': ('rbf', 36, 40, 65, 0, False),
        'rbf-t2-M20-D40-B36': ('rbf', 20, 40, 36, 2, False),
        'rbf-t2-M20-D40-B36-nomean': ('rbf', 20, 40, 36, 2, True),
        'matern32-M20-D2-B33': ('matern32', 20, 2, 33, 0, False),
        'matern52-native-t1-M20-D40-B36': ('matern52n', 20, 40, 36, 1, False),
        'dkl-t1-M20-D40-B36': ('dkl', 20, 40, 36, 1, False),
        'gauss-M20-D40-B33': ('gauss', 20, 40, 33, 0, False),
    }[case]
    phi, nu2 = None, 0
    if kind == 'dkl':
        params, prev, x, _, nz, phi = orc.make_dkl_problem(S, F_, C, M, D, B, n_prev, seed=21)
    else:
        params, prev, x, _, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=n_prev, seed=11 + n_prev + D,
                                                  kind='wtoy' if D == 2 else 'gauss')
    hp = dict(prior_log_mean=params['prior_log_mean'], prior_log_logvar=params['prior_log_logvar'])
    if kind == 'dkl':
        kern = DeepRBFKernel(D, **hp)
        kern.phi.load_state_dict(phi)
    elif kind == 'matern32':
        kern, nu2 = MaternKernel(D, nu=1.5, **hp), 3
    elif kind == 'matern52n':
        kern, nu2 = MaternKernel(D, nu=2.5, native=True, **hp), 5
    else:
        kern = RBFKernel(D, **hp)
    lik = GaussianLikelihood(C) if kind == 'gauss' else MulticlassSoftmax(n_f=F_)
    gp = VARGP(params['z'], kern, lik, n_var_samples=S, ep_var_mean=not nomean,
               prev_params=[{k: v.clone() for k, v in p.items()} for p in prev])
    return _fill(gp, params), params, prev, x, {'eps_theta': nz['eps_theta']}, nu2, phi


def _reference(params, prev, x, nz, nu2, phi, dtype, monkeypatch):
    """ref_predict_f with the case's kernel in place of the oracle's RBF."""
    with monkeypatch.context() as m:
        if nu2:
            m.setattr(orc, 'rbf_gram', lambda theta, x, y=None, full_gram=False: matern_gram(theta, x, y, nu2=nu2))
        if phi is not None:
            with orc.deep_kernel({k: v.to(dtype) for k, v in phi.items()}):
                return ref_predict_f(params, prev, x, nz, dtype)
        return ref_predict_f(params, prev, x, nz, dtype)


def _scaled_err(a, a64, scale):
    return ((a.double() - a64).abs() / scale).max().item()


MODEL_CASES = ['rbf-M20-D2-B33', 'rbf-M36-D40-B65', 'rbf-t2-M20-D40-B36', 'rbf-t2-M20-D40-B36-nomean', 'matern32-M20-D2-B33',
               'matern52-native-t1-M20-D40-B36', 'dkl-t1-M20-D40-B36', 'gauss-M20-D40-B33']


@pytest.mark.parametrize('case', MODEL_CASES)
def test_predict_f_full_cov_vs_fp64(case, monkeypatch):
    from vargp_amd import noise
    gp, params, prev, x, nz, nu2, phi = _model(case)
    mu64, cov64, theta64 = _reference(params, prev, x, nz, nu2, phi, torch.float64, monkeypatch)
    mu32, cov32, _ = _one_thread(lambda: _reference(params, prev, x, nz, nu2, phi, torch.float32, monkeypatch))
    S, C, B = mu64.shape
    with noise.inject(**to_dev(nz, DEV)):
        mu, cov = gp.predict_f(x.to(DEV), full_cov=True)
        mu_d, var_d = gp.predict_f(x.to(DEV))
        with torch.no_grad():
            mu_f, var_f = gp(x.to(DEV))
    assert mu.shape == (S, C, B) and cov.shape == (S, C, B, B)
    assert not mu.requires_grad and not cov.requires_grad
    gamma = theta64[:, -1].exp()
    e_cov = _scaled_err(cov.cpu(), cov64, (gamma ** 2).view(S, 1, 1, 1)), _scaled_err(cov32, cov64, (gamma ** 2).view(S, 1, 1, 1))
    e_mu = _scaled_err(mu.cpu(), mu64, gamma.view(S, 1, 1)), _scaled_err(mu32, mu64, gamma.view(S, 1, 1))
    print(f'{case}: cov err {e_cov[0]:.2e} (fp32 host {e_cov[1]:.2e}), mu err {e_mu[0]:.2e} (fp32 host {e_mu[1]:.2e})')
    assert e_cov[0] <= RTOL_SCALAR + 2.0 * e_cov[1], e_cov
    assert e_mu[0] <= RTOL_SCALAR + 2.0 * e_mu[1], e_mu
    assert torch.equal(cov, cov.mT)
    # without full_cov: exactly what the model's forward returns under no_grad with the same noise
    assert torch.equal(mu_d, mu_f) and torch.equal(var_d, var_f)


# -- 4. sample_f ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['rbf-M20-D2-B33', 'rbf-t2-M20-D40-B36'])
def test_sample_f(case):
    from vargp_amd import noise
    from vargp_amd.ops import JITTER
    gp, params, prev, x, nz, _, _ = _model(case)
    xd = x.to(DEV)
    n = 4
    with noise.inject(**to_dev(nz, DEV)):
        mu, cov = gp.predict_f(xd, full_cov=True)
        S, C, B = mu.shape
        # eps = 0: the mean, exactly
        with noise.inject(eps_fs=torch.zeros(1, S, C, B, device=DEV)):
            f0 = gp.sample_f(xd)
        assert f0.shape == (1, S, C, B) and torch.equal(f0[0], mu)
        eps = torch.randn(n, S, C, B, generator=torch.Generator().manual_seed(3))
        with noise.inject(eps_fs=eps.to(DEV)):
            f = gp.sample_f(xd, n_samples=n)
        # no injection: fresh noise per call
        fa, fb = gp.sample_f(xd, n_samples=2), gp.sample_f(xd, n_samples=2)
    assert f.shape == (n, S, C, B) and fa.shape == (2, S, C, B) and not f.requires_grad
    assert not torch.equal(fa, fb)

    # the covariance the device produced, factorised on the host: fp64 is the reference, fp32 the yardstick of the rule
    def host(dtype):
        c = cov.cpu().to(dtype)
        L = torch.linalg.cholesky(c + JITTER * torch.eye(B, dtype=dtype))
        return mu.cpu().to(dtype).unsqueeze(0) + (L.unsqueeze(0) @ eps.to(dtype).unsqueeze(-1)).squeeze(-1)
    f64 = host(torch.float64)
    f32 = _one_thread(lambda: host(torch.float32))
    theta = orc.sample_hypers(params['log_mean'].double(), params['log_logvar'].double(), nz['eps_theta'].double())
    gamma = theta[:, -1].exp().view(1, S, 1, 1)
    e_hip, e_32 = _scaled_err(f.cpu(), f64, gamma), _scaled_err(f32, f64, gamma)
    print(f'{case}: sample err {e_hip:.2e} (fp32 host {e_32:.2e})')
    assert e_hip <= RTOL_SCALAR + 2.0 * e_32, (e_hip, e_32)
