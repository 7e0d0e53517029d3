"""The fp64 reference of VARGP.predict_f(x, full_cov=True) -- the full predictive covariance and mean of the latent functions at
one block of points -- built from the oracle's functions, and its own validation on the CPU:

    theta = sample_hypers;  q(u_<=t | theta) = compute_q (previous tasks) or (u_mean, Lu Lu^T)
    Lz = chol(Kzz + eps I),  P = Lz^-1 Kzx,  W = (Lz^-1 chol(S + eps I))^T P
    Sigma = K(x, x) - P^T P + W^T W,   mu = P^T Lz^-1 m

tests/test_hip_predict_f.py holds the device code to this reference.  Here the reference itself is pinned, in fp64, to the two
restated formulas of the original that contain it: the variance of linear_marginal_diag (its diagonal) and the lower-right
block of linear_joint with V = the conditional's covariance (the whole matrix, up to the jitter that only the marginal adds
to S: A (S + eps I) A^T - A S A^T = eps A A^T with A = P^T Lz^-1)."""
import pytest
import torch

from oracle import vargp_oracle as orc


def _cast(t, dtype):
    if isinstance(t, torch.Tensor):
        return t.to(dtype) if t.is_floating_point() else t
    if isinstance(t, dict):
        return {k: _cast(v, dtype) for k, v in t.items()}
    if isinstance(t, (list, tuple)):
        return type(t)(_cast(v, dtype) for v in t)
    return t


def ref_predict_f(params, prev, x, nz, dtype=torch.float64, parts=False):
    """-> mu (S, C, B), Sigma (S, C, B, B), theta (S, D+1) in `dtype`.  The kernel is whatever orc.rbf_gram is at the time of the
    call (a test of a Matern model patches it; a deep-kernel test calls this inside orc.deep_kernel(phi)).
    parts=True: also a dict of the intermediate factors."""
    params, prev, x, nz = _cast(params, dtype), _cast(prev, dtype), _cast(x, dtype), _cast(nz, dtype)
    theta = orc.sample_hypers(params['log_mean'], params['log_logvar'], nz['eps_theta'])
    if prev:
        _, _, mu_leq, S_leq, z_leq, _, _ = orc.compute_q(theta, params, prev)
    else:
        mu_leq, z_leq = params['u_mean'], params['z']
        S_leq = orc.llt(orc.vec2tril(params['u_tril_vec']))
    xe = x.unsqueeze(0).expand(z_leq.shape[0], -1, -1)
    Kzz = orc.rbf_gram(theta, z_leq)
    Kzx = orc.rbf_gram(theta, z_leq, xe)
    Kxx = orc.rbf_gram(theta, xe)
    Lz = orc.chol(Kzz)
    P = orc._lsolve(Lz, Kzx)
    W = orc._lsolve(Lz, orc.chol(S_leq).expand(*Lz.shape)).mT @ P
    Sigma = Kxx - P.mT @ P + W.mT @ W
    mu = (P.mT @ orc._lsolve(Lz, mu_leq.expand(*Lz.shape[:-1], 1))).squeeze(-1)
    if parts:
        return mu, Sigma, theta, dict(mu_leq=mu_leq, S_leq=S_leq, Kzz=Kzz, Kzx=Kzx, Kxx=Kxx, Lz=Lz, P=P)
    return mu, Sigma, theta


def _rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


# (S, F, C, M, D, B): the 2-D well-separated toy (B not a multiple of 32) and a 40-dimensional problem
SHAPES = [(2, 3, 3, 20, 2, 33), (2, 3, 3, 20, 40, 36)]


@pytest.mark.parametrize('n_prev', [0, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'M%d-D%d-B%d' % s[3:])
def test_reference_is_the_marginal_of_the_original_formulas(shape, n_prev):
    S, F_, C, M, D, B = shape
    params, prev, x, _, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=n_prev, seed=5 + n_prev, kind='wtoy' if D == 2 else 'gauss')
    mu, Sigma, theta, f = ref_predict_f(params, prev, x, nz, parts=True)
    assert mu.shape == (S, C, B) and Sigma.shape == (S, C, B, B) and Sigma.dtype == torch.float64

    # its diagonal (and its mean): linear_marginal_diag
    m_leq = f['mu_leq'].expand(S, C, -1, 1)
    S_leq = f['S_leq'].expand(S, C, *f['S_leq'].shape[-2:])
    mu_d, var_d, _, _ = orc.linear_marginal_diag(m_leq, S_leq, f['Kzz'], f['Kzx'], orc.rbf_diag(theta))
    e_var, e_mu = _rel(Sigma.diagonal(dim1=-2, dim2=-1), var_d), _rel(mu, mu_d)
    print(f'diag vs linear_marginal_diag: var {e_var:.2e}  mu {e_mu:.2e}')
    assert e_var <= 1e-10 and e_mu <= 1e-10

    # the whole matrix: lower-right block of linear_joint with V = the conditional's covariance, b = 0 -- whose S carries no
    # jitter, so the difference is exactly JITTER A A^T = JITTER P^T (Lz^-1 Lz^-T) P
    _, V = orc.gp_cond(m_leq, f['Kxx'], f['Lz'], f['P'])
    mu_j, Sig_j, _, _ = orc.linear_joint(m_leq, S_leq, f['Kzx'], f['Kzz'], V, torch.zeros(S, C, B, 1, dtype=torch.float64))
    Mt = f['Kzz'].shape[-1]
    Tz = orc._lsolve(f['Lz'], torch.eye(Mt, dtype=torch.float64).expand(S, C, Mt, Mt))
    A = f['P'].mT @ Tz
    want = Sig_j[..., Mt:, Mt:] + orc.JITTER * (A @ A.mT)
    e_cov, e_muj = _rel(Sigma, want), _rel(mu, mu_j[..., Mt:, 0])
    print(f'vs linear_joint + JITTER A A^T: cov {e_cov:.2e}  mu {e_muj:.2e}')
    assert e_cov <= 1e-10 and e_muj <= 1e-10
    # (and the jitter term is not nothing: without it the two differ by far more than the tolerance)
    assert _rel(Sigma, Sig_j[..., Mt:, Mt:]) > 1e-8


def test_predictive_cov_refuses_cpu_tensors():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    S, C, Mt, B, D = 2, 3, 5, 7, 4
    with pytest.raises(VargpHipError):
        ops.predictive_cov(torch.zeros(S, D + 1), torch.zeros(B, D), torch.zeros(S, C, Mt, B), torch.zeros(S, C, Mt, B), 0)


def test_new_entries_are_bound():
    from vargp_amd import _lib
    from vargp_amd.vargp import VARGP
    assert {'vargp_predictive_cov', 'vargp_predictive_cov_workspace_bytes'} <= set(_lib.EXPORTS)
    assert callable(VARGP.predict_f) and callable(VARGP.sample_f)
    lib = _lib.lib()
    assert lib.vargp_predictive_cov_workspace_bytes(2, 33, 40) >= 4 * (2 * 40 + 2 + 2 * 33 + 2 * 33 * 40)
