"""The closed-form optimal q(u) of a Gaussian-likelihood model (vargp_amd/collapsed.py, VARGP.fit_q_), the part that needs no GPU:
a dense restatement of the moments (csrc/moments.hip) and of the solver in plain torch, in any dtype -- what
tests/test_hip_collapsed.py measures the device against -- checked here in fp64 for what the derivation claims: at the restated
optimum the gradient of the EVALUATED bound, E_q log N(y | f, 1 / beta) - KL(q(v_t) || N(0, I)) summed point by point, vanishes,
and the closed-form value equals the evaluated one.  Then the C-ABI entry's argument checks and workspace bound, and the argument
checks of fit_q_ and create_reg(q_init=)."""
import ctypes
import math

import pytest
import torch

JITTER = 1e-4


# -- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_kernel(xa, xb, theta, nu2):
    """k(x, y) = gamma^2 f(r), r^2 = sum_d ((x_d - y_d) / lengthscale_d)^2; xa (.., n, D) against xb (.., m, D) -> (.., n, m) in the
    dtype of the inputs.  nu2: 0 = RBF exp(-r^2 / 2); 1, 3, 5 = Matern nu = nu2 / 2."""
    ls, g2 = theta[:-1].exp(), (2.0 * theta[-1]).exp()
    r2 = (((xa.unsqueeze(-2) - xb.unsqueeze(-3)) / ls) ** 2).sum(-1)
    if nu2 == 0:
        return g2 * (-0.5 * r2).exp()
    a = (nu2 * r2).sqrt()
    poly = {1: 1.0, 3: 1.0 + a, 5: 1.0 + a + (5.0 / 3.0) * r2}[nu2]
    return g2 * poly * (-a).exp()


def ref_moments(theta, Z, X, w, y, nu2, dtype=torch.float64):
    """Z (G, Mt, D), X (N, D), w (G, N) or None, y (G, N) -> Phi (G, Mt, Mt), c (G, Mt), sums (G, 2), dense."""
    theta, Z, X, y = theta.to(dtype), Z.to(dtype), X.to(dtype), y.to(dtype)
    w = torch.ones_like(y) if w is None else w.to(dtype)
    K = ref_kernel(Z, X.unsqueeze(0), theta, nu2)                                  # (G, Mt, N)
    Phi = (K * w.unsqueeze(-2)) @ K.mT
    c = (K * (w * y).unsqueeze(-2)).sum(-1)
    return Phi, c, torch.stack([w.sum(-1), (w * y * y).sum(-1)], -1)


def ref_vec2tril(vec, M):
    """packed (C, M (M + 1) / 2), row-major lower triangle -> (C, M, M) with softplus on the diagonal (gp_utils.vec2tril)."""
    i, j = torch.tril_indices(M, M)
    L = vec.new_zeros(vec.shape[0], M, M)
    L[:, i, j] = vec
    d = torch.arange(M)
    L[:, d, d] = torch.nn.functional.softplus(L[:, d, d])
    return L


def ref_whiten(theta, z_all, prev, nu2, eps=JITTER, dtype=torch.float64):
    """z_all (C, Mt, D): the inducing points of all tasks in task order; prev: [dict(u_mean (C, n, 1), u_tril (C, n, n))] of the
    frozen tasks.  -> L, T (C, Mt, Mt), a_< (C, n_<), [H_i] -- the whitened posterior of the frozen tasks (gp_utils.block_joint)."""
    theta, z_all = theta.to(dtype), z_all.to(dtype)
    Mt = z_all.shape[-2]
    eye = torch.eye(Mt, dtype=dtype)
    L = torch.linalg.cholesky(ref_kernel(z_all, z_all, theta, nu2) + eps * eye)
    T = torch.linalg.solve_triangular(L, eye.expand_as(L), upper=False)
    a, H, o = [], [], 0
    for p in prev:
        n = p['u_mean'].shape[-2]
        T_ii = T[:, o:o + n, o:o + n]
        a.append((T_ii @ p['u_mean'].to(dtype)).squeeze(-1))
        H.append(T_ii @ p['u_tril'].to(dtype))
        o += n
    return L, T, (torch.cat(a, -1) if a else L.new_zeros(L.shape[0], 0)), H


def ref_fit(theta, z_all, prev, x, y, w, obs_log_var, nu2, temper=1.0, eps=JITTER, dtype=torch.float64):
    """The formulas of collapsed.py, dense.  y (C, N), w (C, N) or None, obs_log_var (C,).  -> dict: u_mean (C, M), u_tril (C, M, M),
    bound (C,), a_t (C, M), Sigma_t (C, M, M), kl (C,) = KL(q(v_t) || N(0, I)) at the optimum."""
    L, T, a_lt, H = ref_whiten(theta, z_all, prev, nu2, eps, dtype)
    Phi, c, sums = ref_moments(theta, z_all, x, w, y, nu2, dtype)
    n_lt = a_lt.shape[-1]
    M = z_all.shape[-2] - n_lt
    A = T @ Phi @ T.mT
    tc = (T @ c.unsqueeze(-1)).squeeze(-1)
    sw, syy = sums[:, 0], sums[:, 1]
    beta = temper * (-obs_log_var.to(dtype)).exp()
    g2 = (2.0 * theta[-1].to(dtype)).exp()
    mv = lambda B, v: (B @ v.unsqueeze(-1)).squeeze(-1)
    b_t = tc[:, n_lt:] - mv(A[:, n_lt:, :n_lt], a_lt)
    Bm = torch.eye(M, dtype=dtype) + beta.view(-1, 1, 1) * A[:, n_lt:, n_lt:]
    Sigma = torch.linalg.inv(Bm)
    Sigma = 0.5 * (Sigma + Sigma.mT)
    a_t = beta.unsqueeze(-1) * mv(Sigma, b_t)
    L_tt = L[:, n_lt:, n_lt:]
    S_u = L_tt @ Sigma @ L_tt.mT
    u_tril = torch.linalg.cholesky(0.5 * (S_u + S_u.mT))
    trHAH, o = torch.zeros_like(sw), 0
    for H_i in H:
        n = H_i.shape[-1]
        trHAH = trHAH + (H_i * (A[:, o:o + n, o:o + n] @ H_i)).sum((-2, -1))
        o += n
    fixed = syy - 2.0 * (a_lt * tc[:, :n_lt]).sum(-1) + (a_lt * mv(A[:, :n_lt, :n_lt], a_lt)).sum(-1) + g2 * sw \
        - A.diagonal(dim1=-2, dim2=-1).sum(-1) + trHAH
    quad = (b_t * mv(Sigma, b_t)).sum(-1)
    logdet = torch.linalg.slogdet(Bm)[1]
    bound = -0.5 * sw * (2.0 * math.pi / beta).log() - 0.5 * beta * fixed + 0.5 * beta ** 2 * quad - 0.5 * logdet
    kl = 0.5 * (Sigma.diagonal(dim1=-2, dim2=-1).sum(-1) + (a_t * a_t).sum(-1) - M + logdet)
    return dict(u_mean=mv(L_tt, a_t), u_tril=u_tril, bound=bound, a_t=a_t, Sigma_t=Sigma, kl=kl)


def ref_bound_evaluated(theta, z_all, prev, x, y, w, obs_log_var, nu2, a_t, H_t, temper=1.0, eps=JITTER):
    """The bound for ANY q(v_t) = N(a_t, H_t H_t^T), fp64, summed point by point from the dense K(z, x): no moments, no closed form.
    E_q (y_n - f_n)^2 = (y_n - p_n^T a)^2 + |H^T p_n|^2 + gamma^2 - |p_n|^2, p_n = T k_n, with a = [a_<; a_t], H = blockdiag."""
    dtype = torch.float64
    L, T, a_lt, H = ref_whiten(theta, z_all, prev, nu2, eps, dtype)
    M = a_t.shape[-1]
    theta, y = theta.to(dtype), y.to(dtype)
    w = torch.ones_like(y) if w is None else w.to(dtype)
    beta = (temper * (-obs_log_var.to(dtype)).exp()).unsqueeze(-1)
    P = T @ ref_kernel(z_all.to(dtype), x.to(dtype).unsqueeze(0), theta, nu2)      # (C, Mt, N)
    a = torch.cat([a_lt, a_t], -1)
    Hb = torch.stack([torch.block_diag(*[Hi[c] for Hi in H], H_t[c]) for c in range(a.shape[0])])
    mean = (P * a.unsqueeze(-1)).sum(-2)
    var = ((Hb.mT @ P) ** 2).sum(-2) + (2.0 * theta[-1]).exp() - (P * P).sum(-2)
    ell = (w * (-0.5 * (2.0 * math.pi / beta).log() - 0.5 * beta * ((y - mean) ** 2 + var))).sum(-1)
    S = H_t @ H_t.mT
    kl = 0.5 * (S.diagonal(dim1=-2, dim2=-1).sum(-1) + (a_t * a_t).sum(-1) - M - torch.linalg.slogdet(S)[1])
    return ell - kl


def ref_predict(theta, z_all, means, trils, xs, nu2, eps=JITTER, dtype=torch.float64):
    """The model's predictive moments at theta (VARGP.forward restated: block_joint, then linear_marginal_diag with its jitter on
    S): means [(C, n, 1)], trils [(C, n, n)] of all tasks, xs (B, D) -> mu, var (C, B)."""
    prev = [dict(u_mean=m, u_tril=t) for m, t in zip(means, trils)]
    L, T, a, H = ref_whiten(theta, z_all, prev, nu2, eps, dtype)
    Mt = z_all.shape[-2]
    LH = L @ torch.stack([torch.block_diag(*[Hi[c] for Hi in H]) for c in range(L.shape[0])])
    LS = torch.linalg.cholesky(LH @ LH.mT + eps * torch.eye(Mt, dtype=dtype))
    P = T @ ref_kernel(z_all.to(dtype), xs.to(dtype).unsqueeze(0), theta.to(dtype), nu2)
    W = (T @ LS).mT @ P
    return (P * a.unsqueeze(-1)).sum(-2), (2.0 * theta[-1].to(dtype)).exp() - (P * P).sum(-2) + (W * W).sum(-2)


def make_problem(C, M, n_prev, D, N, seed, ell=0.8, weights=False):
    """A regression problem in float32: inputs ~ N(0, I), targets = a smooth function + noise per output, n_prev frozen tasks
    with random q(u).  -> dict(theta, z_all (C, Mt, D), prev [dict(z, u_mean, u_tril_vec, u_tril)], x, y (C, N), w, obs_log_var)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, D, generator=g)
    y = torch.stack([torch.sin(1.5 * x[:, 0] + c) + 0.3 * x[:, -1] for c in range(C)]) + 0.1 * torch.randn(C, N, generator=g)
    z = [torch.randn(C, M, D, generator=g) for _ in range(n_prev + 1)]
    prev = []
    for i in range(n_prev):
        vec = 0.3 * torch.randn(C, M * (M + 1) // 2, generator=g)
        prev.append(dict(z=z[i], u_mean=0.5 * torch.randn(C, M, 1, generator=g), u_tril_vec=vec, u_tril=ref_vec2tril(vec, M)))
    theta = torch.cat([math.log(ell * math.sqrt(D)) + 0.1 * torch.randn(D, generator=g), torch.tensor([math.log(0.9)])])
    w = torch.rand(C, N, generator=g) + 0.5 if weights else None
    return dict(theta=theta, z_all=torch.cat(z, -2), prev=prev, x=x, y=y, w=w, obs_log_var=torch.linspace(-3.0, -2.0, C))


@pytest.mark.parametrize('nu2', [0, 3])
@pytest.mark.parametrize('t', [0, 2])
def test_gradient_vanishes_and_closed_form_equals_the_evaluated_bound(t, nu2):
    """M = 5, D = 3, N = 40, two outputs, weights and temper != 1: at (a_t, chol(Sigma_t)) of the restatement autograd's gradient of
    the evaluated bound is below 1e-9 in every entry, and the closed-form bound is the evaluated one."""
    pr = make_problem(2, 5, t, 3, 40, seed=10 + t, weights=True)
    args = (pr['theta'], pr['z_all'], pr['prev'], pr['x'], pr['y'], pr['w'], pr['obs_log_var'], nu2)
    fit = ref_fit(*args, temper=0.7)
    a_t = fit['a_t'].clone().requires_grad_(True)
    H_raw = torch.linalg.cholesky(fit['Sigma_t']).clone().requires_grad_(True)
    val = ref_bound_evaluated(*args, a_t, H_raw.tril(), temper=0.7)
    ga, gH = torch.autograd.grad(val.sum(), (a_t, H_raw))
    print(f't={t} nu2={nu2}: |grad a| {ga.abs().max().item():.2e} |grad H| {gH.abs().max().item():.2e}, bound {fit["bound"].tolist()} '
          f'evaluated {val.tolist()}')
    assert ga.abs().max().item() < 1e-9 and gH.abs().max().item() < 1e-9
    assert torch.allclose(fit['bound'], val.detach(), rtol=1e-11, atol=0.0)
    # a maximum: any other q(v_t) is worse
    worse = ref_bound_evaluated(*args, fit['a_t'] + 0.01, 1.1 * torch.linalg.cholesky(fit['Sigma_t']), temper=0.7)
    assert bool((worse < val.detach()).all())
    # the KL term as the closed form states it
    S = fit['Sigma_t']
    assert torch.allclose(fit['kl'], 0.5 * (S.diagonal(dim1=-2, dim2=-1).sum(-1) + (fit['a_t'] ** 2).sum(-1) - 5
                                            - torch.linalg.slogdet(S)[1]), rtol=1e-10)
    # u_tril is the factor of L_tt Sigma_t L_tt^T and u_mean = L_tt a_t: T_tt maps them back
    _, T, _, _ = ref_whiten(pr['theta'], pr['z_all'], pr['prev'], nu2)
    T_tt = T[:, -5:, -5:]
    assert torch.allclose((T_tt @ fit['u_mean'].unsqueeze(-1)).squeeze(-1), fit['a_t'], rtol=0, atol=1e-9)
    Hh = T_tt @ fit['u_tril']
    assert torch.allclose(Hh @ Hh.mT, S, rtol=0, atol=1e-9)


def test_exact_gp_when_the_inducing_points_are_the_data():
    """z = x (N = 12), first task, unit weights: the fitted predictive mean is the exact GP posterior mean up to the jitter."""
    pr = make_problem(1, 12, 0, 2, 12, seed=3)
    z = pr['x'].unsqueeze(0)
    fit = ref_fit(pr['theta'], z, [], pr['x'], pr['y'], None, pr['obs_log_var'], 0)
    xs = torch.randn(7, 2, generator=torch.Generator().manual_seed(1))
    mu, _ = ref_predict(pr['theta'], z, [fit['u_mean'].unsqueeze(-1)], [fit['u_tril']], xs, 0)
    th, x64 = pr['theta'].double(), pr['x'].double()
    Kxx = ref_kernel(x64, x64, th, 0) + pr['obs_log_var'].double().exp() * torch.eye(12, dtype=torch.float64)
    exact = ref_kernel(xs.double(), x64, th, 0) @ torch.linalg.solve(Kxx, pr['y'][0].double())
    assert (mu[0] - exact).abs().max().item() < 5e-3


# -- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    from vargp_amd import _lib
    for name in ('vargp_gram_moments', 'vargp_gram_moments_workspace_bytes', 'vargp_gram_moments_chunks'):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)


def test_workspace_does_not_grow_with_the_data():
    """Per-chunk partials only: the chunk count is capped, so 2000 times the points need the same bytes; the stated bound holds."""
    from vargp_amd._lib import lib
    ws, chunks = lib().vargp_gram_moments_workspace_bytes, lib().vargp_gram_moments_chunks
    for G, Mt in ((1, 100), (1, 500), (10, 100), (3, 2048)):
        nt = (Mt + 63) // 64
        ntri = nt * (nt + 1) // 2
        big = [ws(G, Mt, N, 8) for N in (10 ** 6, 10 ** 7, 2 * 10 ** 9)]
        assert min(big) > 0 and max(big) <= 1.02 * min(big)           # (the chunk length is rounded to 64 columns: not exactly equal)
        for N in (1, 1000, 10 ** 6, 2 * 10 ** 9):
            n = chunks(G, Mt, N, 8)
            assert 1 <= n <= 1024 and n * G * ntri <= 1024 + G * ntri and n <= (N + 255) // 256
            assert ws(G, Mt, N, 8) <= (1024 + G * ntri) * 17000 + 1024
    assert chunks(1, 15, 1000, 3) > 1 and chunks(1, 15, 64, 3) == 1
    assert ws(0, 5, 5, 5) == 0 and chunks(1, 0, 5, 5) == 0
    assert ws(1, 100, 10 ** 6, 8) == ws(1, 100, 10 ** 6, 784)                      # no panel buffer at any D


def test_cabi_argument_errors_before_any_launch():
    """A null pointer other than w, a size < 1, a kernel code outside the four, G > 65535 or a short workspace: VARGP_EINVAL (-1)
    with host memory for pointers -- nothing is launched, so no device is touched."""
    from vargp_amd._lib import lib
    L = lib()
    EINVAL = -1
    G, Mt, N, D = 2, 5, 9, 3
    need = L.vargp_gram_moments_workspace_bytes(G, Mt, N, D)
    buf = (ctypes.c_float * (need // 4 + 16))()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)
    fn = L.vargp_gram_moments

    def call(ptrs=None, dims=(G, Mt, N, D), nu2=0, ws=p, ws_bytes=need):
        return fn(*(ptrs or [p] * 8), *dims, nu2, ws, ws_bytes, None)

    for bad in (0, 1, 2, 4, 5, 6, 7):                                # every pointer but w (3)
        assert call([null if q == bad else p for q in range(8)]) == EINVAL
    assert call(ws=null) == EINVAL
    for dims in ((0, Mt, N, D), (G, 0, N, D), (G, Mt, 0, D), (G, Mt, N, 0), (-1, Mt, N, D), (65536, Mt, N, D)):
        assert call(dims=dims, ws_bytes=1 << 40) == EINVAL, dims
    for nu2 in (-1, 2, 4, 6):
        assert call(nu2=nu2) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and call(ws_bytes=0) == EINVAL
    assert b'gram_moments' in L.vargp_last_error()


# -- the Python surface -------------------------------------------------------------------------------------------------------------
class _Data:
    def __init__(self, x, targets):
        self.x, self.targets = x, targets

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.targets[i]


def test_fit_q_names_what_it_supports():
    from vargp_amd._lib import VargpHipError
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    clf = VARGP.create_clf(_Data(x, torch.arange(40) % 3), M=4)
    with pytest.raises(ValueError, match='GaussianLikelihood'):
        clf.fit_q_(x, torch.arange(40) % 3)
    reg = _Data(x, x[:, 0].clone())
    with pytest.raises(ValueError, match='ep_var_mean=True'):
        VARGP.create_reg(reg, M=4, ep_var_mean=False).fit_q_(x, reg.targets)
    with pytest.raises(ValueError, match='GaussianLikelihood'):
        VARGP.create_reg(reg, M=4, likelihood='studentt').fit_q_(x, reg.targets)
    with pytest.raises(VargpHipError):                              # a supported model on the host: no CPU path
        VARGP.create_reg(reg, M=4).fit_q_(x, reg.targets)
    with pytest.raises(ValueError, match='q_init'):
        VARGP.create_reg(reg, M=4, q_init='best')
    with pytest.raises(ValueError, match='gaussian'):
        VARGP.create_reg(reg, M=4, likelihood='poisson', q_init='optimal')


def test_ops_refuse_cpu_tensors():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    with pytest.raises(VargpHipError):
        ops.gram_moments(torch.zeros(4), torch.randn(1, 5, 3), torch.randn(9, 3), None, torch.randn(1, 9))
    assert ops.gram_moments_chunks(1, 15, 1000, 3) > 1


def test_inv_softplus_round_trip():
    from vargp_amd.collapsed import inv_softplus
    d = torch.tensor([1e-6, 1e-3, 0.5, 1.0, 19.0, 25.0, 300.0], dtype=torch.float64)
    assert torch.allclose(torch.nn.functional.softplus(inv_softplus(d)), d, rtol=1e-12, atol=0.0)
