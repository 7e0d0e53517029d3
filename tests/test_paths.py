"""The fp64 reference of VARGP.sample_paths -- pathwise (Matheron) samples of the posterior over the latent functions -- built
from the oracle's functions, and its own validation on the CPU:

    Phi_s(x) = gamma_s / sqrt(R) [cos p | sin p],  p = (x / lengthscale_s) omega^T
    g(x) = Phi_s(x) w,   r = Lz^-1 m + G eps_u - Lz^-1 g(z),   V = Lz^-T r,   f(x) = g(x) + K(x, z) V

tests/test_hip_paths.py holds the device code to this reference.  Here the reference itself is pinned, in fp64, to
ref_predict_f (tests/test_predict_f.py): f is affine in the noise (w, eps_u), its value at zero noise is the predictive mean and
its Jacobian J satisfies J J^T = Phi~ Phi~^T + W^T W with Phi~ = Phi(x) - P^T Lz^-1 Phi(z) -- the random-feature estimate of
K(x, x) - P^T P, plus predict_f's W^T W.  And the spectral laws of kernels.py (pure torch, CPU) are held to the kernels they
belong to: Phi Phi^T -> K at the Monte-Carlo rate."""
import math

import pytest
import torch

from oracle import vargp_oracle as orc
from test_predict_f import SHAPES, _cast, ref_predict_f


def _features(x):
    """The inputs of the RBF head inside orc.deep_kernel(phi); x itself otherwise."""
    return x if orc._feature_map is None else orc.deep_features(orc._feature_map, x)


def ref_phi(theta, x, omega):
    """Phi_s(x): theta (S, D+1), x (..., n, D), omega (R, D) -> (S, ..., n, 2R)."""
    S, R = theta.shape[0], omega.shape[0]
    x = _features(x)
    th = theta.reshape(S, *([1] * (x.dim() - 1)), -1)
    p = (x.unsqueeze(0) / th[..., :-1].exp()) @ omega.mT
    return th[..., -1:].exp() / math.sqrt(R) * torch.cat([p.cos(), p.sin()], dim=-1)


def ref_paths(params, prev, x, nz, omega, coef, eps_u, dtype=torch.float64):
    """-> f (N, S, C, B), theta (S, D+1) in `dtype`: the paths with weights coef (S, C, 2R, N) and inducing noise eps_u
    (S, C, Mt, N) at x (B, D).  The kernel is whatever orc.rbf_gram is at the time of the call, as for ref_predict_f (a deep
    kernel: call inside orc.deep_kernel(phi); omega then lives in the feature space)."""
    params, prev, x, nz = _cast(params, dtype), _cast(prev, dtype), _cast(x, dtype), _cast(nz, dtype)
    omega, coef, eps_u = omega.to(dtype), coef.to(dtype), eps_u.to(dtype)
    theta = orc.sample_hypers(params['log_mean'], params['log_logvar'], nz['eps_theta'])
    if prev:
        _, _, mu_leq, S_leq, z_leq, _, _ = orc.compute_q(theta, params, prev)
    else:
        mu_leq, z_leq = params['u_mean'], params['z']
        S_leq = orc.llt(orc.vec2tril(params['u_tril_vec']))
    xe = x.unsqueeze(0).expand(z_leq.shape[0], -1, -1)
    Lz = orc.chol(orc.rbf_gram(theta, z_leq))
    Kzx = orc.rbf_gram(theta, z_leq, xe)
    a = orc._lsolve(Lz, mu_leq.expand(*Lz.shape[:-1], 1))
    G = orc._lsolve(Lz, orc.chol(S_leq).expand(*Lz.shape))
    r = a + G @ eps_u - orc._lsolve(Lz, ref_phi(theta, z_leq, omega) @ coef)
    V = torch.linalg.solve_triangular(Lz.mT, r, upper=True)
    f = ref_phi(theta, x, omega).unsqueeze(1) @ coef + Kzx.mT @ V               # (S, C, B, N)
    return f.permute(3, 0, 1, 2), theta


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize('n_prev', [0, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'M%d-D%d-B%d' % s[3:])
def test_reference_mean_and_covariance(shape, n_prev):
    S, F_, C, M, D, B = shape
    R = 8
    params, prev, x, _, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=n_prev, seed=5 + n_prev, kind='wtoy' if D == 2 else 'gauss')
    Mt = (n_prev + 1) * M
    omega = torch.randn(R, D, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    # column 0: no noise; then the unit vectors of w, then those of eps_u
    N = 1 + 2 * R + Mt
    coef = torch.zeros(S, C, 2 * R, N, dtype=torch.float64)
    eps_u = torch.zeros(S, C, Mt, N, dtype=torch.float64)
    coef[..., 1:1 + 2 * R] = torch.eye(2 * R, dtype=torch.float64)
    eps_u[..., 1 + 2 * R:] = torch.eye(Mt, dtype=torch.float64)
    f, theta = ref_paths(params, prev, x, nz, omega, coef, eps_u)
    assert f.shape == (N, S, C, B) and f.dtype == torch.float64

    mu, Sigma, theta_p, parts = ref_predict_f(params, prev, x, nz, parts=True)
    assert torch.equal(theta, theta_p)
    e_mu = _rel(f[0], mu)
    J = (f[1:] - f[0]).permute(1, 2, 3, 0)                                      # (S, C, B, 2R + Mt)
    P, Lz = parts['P'], parts['Lz']
    z_leq = torch.cat([p['z'] for p in prev] + [params['z']], dim=-2).double()
    Phi_t = ref_phi(theta, x.double(), omega).unsqueeze(1) - P.mT @ orc._lsolve(Lz, ref_phi(theta, z_leq, omega))
    WtW = Sigma - parts['Kxx'] + P.mT @ P                                       # ref_predict_f's W^T W
    e_cov = _rel(J @ J.mT, Phi_t @ Phi_t.mT + WtW)
    print(f'mean vs ref_predict_f {e_mu:.2e}; J J^T vs Phi~ Phi~^T + W^T W {e_cov:.2e}')
    assert e_mu <= 1e-10 and e_cov <= 1e-10
    # (and both parts of the covariance are there: either one alone is far off)
    assert _rel(J @ J.mT, WtW) > 1e-3 and _rel(J @ J.mT, Phi_t @ Phi_t.mT) > 1e-3


@pytest.mark.parametrize('D', [2, 40])
@pytest.mark.parametrize('nu2', [0, 1, 3, 5])
def test_spectral_frequencies_reproduce_the_kernel(nu2, D):
    """max |Phi Phi^T - K| / gamma^2 <= 6.45 / sqrt(R): an entry of Phi Phi^T / gamma^2 is the mean of R independent
    cos((x - y) / lengthscale . omega_r) in [-1, 1] with expectation k(x, y) / gamma^2, so by Hoeffding's inequality it is off
    by more than t with probability <= 2 exp(-R t^2 / 2); t = 6.45 / sqrt(R) over the 33 32 / 2 + 17 ~ 545 distinct entries of
    the two hyper-samples' matrices gives a failure probability of 1e-6.  A wrong spectral law converges elsewhere."""
    from test_hip_predict_f import _gram, _op_inputs
    from vargp_amd.kernels import MaternKernel, RBFKernel
    R, B = 4096, 33
    theta, X, _, _ = _op_inputs(B, 1, D, seed=100 + 10 * nu2 + D)
    kern = RBFKernel(D) if nu2 == 0 else MaternKernel(D, nu=nu2 / 2)
    torch.manual_seed(1234 + nu2 + D)
    omega = kern.spectral_frequencies(R, 'cpu')
    assert omega.shape == (R, D) and omega.dtype == torch.float32 and not omega.is_cuda
    theta, X, omega = theta.double(), X.double(), omega.double()
    Phi = ref_phi(theta, X, omega)                                              # (S, B, 2R)
    K = _gram(theta, X, nu2).squeeze(1)
    g2 = (2.0 * theta[:, -1]).exp().view(-1, 1, 1)
    err = ((Phi @ Phi.mT - K).abs() / g2).max().item()
    print(f'nu2={nu2} D={D}: max |Phi Phi^T - K| / gamma^2 = {err:.4f} (bound {6.45 / math.sqrt(R):.4f}); K / gamma^2 in '
          f'[{(K / g2).min().item():.3f}, {(K / g2).max().item():.3f}]')
    assert err <= 6.45 / math.sqrt(R)


def test_spectral_frequencies_noise_by_name():
    """The draws come through noise.draw by name: rff_omega (R, D) for every kernel, rff_mix (R, nu2) for the Matern ones only."""
    from vargp_amd import noise
    from vargp_amd.kernels import MaternKernel, RBFKernel
    R, D = 6, 3
    g = torch.randn(R, D)
    with noise.inject(rff_omega=g):
        assert torch.equal(RBFKernel(D).spectral_frequencies(R, 'cpu'), g)
        mix = torch.randn(R, 3)
        with noise.inject(rff_mix=mix):
            om = MaternKernel(D, nu=1.5).spectral_frequencies(R, 'cpu')
    want = g * (3.0 / (mix ** 2).sum(-1, keepdim=True)).sqrt()
    assert torch.allclose(om, want, rtol=1e-6, atol=0)


def test_rff_paths_refuses_cpu_tensors():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    S, C, n, D, R, N = 2, 3, 5, 4, 6, 2
    with pytest.raises(VargpHipError):
        ops.rff_paths(torch.zeros(S, D + 1), torch.zeros(n, D), torch.zeros(R, D), torch.zeros(S, C, 2 * R, N), True)
    with pytest.raises(VargpHipError):
        ops.rff_paths(torch.zeros(S, D + 1), torch.zeros(C, n, D), torch.zeros(R, D), torch.zeros(S, C, 2 * R, N), False)


def test_new_entries_are_bound():
    from vargp_amd import _lib
    from vargp_amd.paths import PosteriorPaths
    from vargp_amd.vargp import VARGP
    assert {'vargp_rff_paths', 'vargp_rff_paths_workspace_bytes'} <= set(_lib.EXPORTS)
    assert callable(VARGP.sample_paths) and callable(PosteriorPaths.__call__)
    # the pre-scaled frequencies of every hyper-sample and its amplitude
    assert _lib.lib().vargp_rff_paths_workspace_bytes(2, 40, 100) >= 4 * (2 * 100 * 40 + 2)
