"""The differentiable collapsed bound (vargp_amd/collapsed.py: collapsed_bound, fit_collapsed_; ops.gram_moments_diff on the fused
backward csrc/moments.hip: vargp_gram_moments_bwd), the part that needs no GPU: the C-ABI entry's symbols, argument checks and
workspace bound; an fp64 restatement of the bound as a differentiable torch function on top of tests/test_collapsed.py's pieces --
the yardstick of tests/test_hip_collapsed_grad.py -- pinned against ref_fit's value and against central differences; the identity
that gives the log-gamma entry of the moments' gradient without a pass over the data; what the Python surface refuses; and the
conditions of the device's fit_collapsed_ test, shown on the restatement with plain gradient ascent."""
import ctypes
import math

import pytest
import torch

from test_collapsed import JITTER, _Data, make_problem, ref_fit, ref_moments, ref_predict, ref_whiten


# -- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_whiten_diff(theta, z_all, prev, nu2, eps=JITTER, dtype=torch.float64):
    """ref_whiten, value for value, with a K(z, z) that autograd can differentiate: ref_kernel takes sqrt(r^2) at r^2 = 0 on the
    diagonal, whose derivative is inf (times 0: NaN for the Matern kernels).  The diagonal is gamma^2 whatever z is, so it is
    computed at r^2 = 1 and replaced."""
    theta, z_all = theta.to(dtype), z_all.to(dtype)
    Mt = z_all.shape[-2]
    eye = torch.eye(Mt, dtype=dtype)
    ls, g2 = theta[:-1].exp(), (2.0 * theta[-1]).exp()
    r2 = (((z_all.unsqueeze(-2) - z_all.unsqueeze(-3)) / ls) ** 2).sum(-1) + eye
    a = (nu2 * r2).sqrt()
    f = (-0.5 * r2).exp() if nu2 == 0 else {1: 1.0, 3: 1.0 + a, 5: 1.0 + a + (5.0 / 3.0) * r2}[nu2] * (-a).exp()
    L = torch.linalg.cholesky(g2 * (f * (1.0 - eye) + eye) + eps * eye)
    T = torch.linalg.solve_triangular(L, eye.expand_as(L), upper=False)
    a, H, o = [], [], 0
    for p in prev:
        n = p['u_mean'].shape[-2]
        T_ii = T[:, o:o + n, o:o + n]
        a.append((T_ii @ p['u_mean'].to(dtype)).squeeze(-1))
        H.append(T_ii @ p['u_tril'].to(dtype))
        o += n
    return L, T, (torch.cat(a, -1) if a else L.new_zeros(L.shape[0], 0)), H


class _MaternOfR2(torch.autograd.Function):
    """f(r^2) of ref_kernel's Matern kernels, value for value, with the closed-form derivative df/dr^2 = -exp(-a) / (2 a) nu2 |
    -(3/2) exp(-a) | -(5/6) (1 + a) exp(-a), a = sqrt(nu2 r^2): autograd's chain through sqrt is inf x 0 = NaN at r^2 = 0 (an
    inducing point ON a data point, as create_reg places them), where the last two are finite; nu = 1/2 has no derivative there
    and gets 0, the convention of csrc/common.h's matern_w."""
    @staticmethod
    def forward(ctx, r2, nu2):
        a = (nu2 * r2).sqrt()
        ctx.save_for_backward(r2, a)
        ctx.nu2 = nu2
        return {1: 1.0, 3: 1.0 + a, 5: 1.0 + a + (5.0 / 3.0) * r2}[nu2] * (-a).exp()

    @staticmethod
    def backward(ctx, g):
        r2, a = ctx.saved_tensors
        if ctx.nu2 == 1:
            d = torch.where(r2 > 0, -0.5 * (-a).exp() / a.clamp_min(1e-300), torch.zeros_like(a))
        else:
            d = -1.5 * (-a).exp() if ctx.nu2 == 3 else -(5.0 / 6.0) * (1.0 + a) * (-a).exp()
        return g * d, None


def ref_moments_diff(theta, Z, X, w, y, nu2, dtype=torch.float64):
    """ref_moments, value for value, on a cross-kernel that autograd can differentiate at coincident points (_MaternOfR2)."""
    theta, Z, X, y = theta.to(dtype), Z.to(dtype), X.to(dtype), y.to(dtype)
    w = torch.ones_like(y) if w is None else w.to(dtype)
    r2 = (((Z.unsqueeze(-2) - X.unsqueeze(0).unsqueeze(-3)) / theta[:-1].exp()) ** 2).sum(-1)
    K = (2.0 * theta[-1]).exp() * ((-0.5 * r2).exp() if nu2 == 0 else _MaternOfR2.apply(r2, nu2))
    Phi = (K * w.unsqueeze(-2)) @ K.mT
    c = (K * (w * y).unsqueeze(-2)).sum(-1)
    return Phi, c, torch.stack([w.sum(-1), (w * y * y).sum(-1)], -1)


def ref_bound(theta, z_all, prev, x, y, w, obs_log_var, nu2, temper=1.0, eps=JITTER, dtype=torch.float64):
    """The collapsed bound (C,) of collapsed.py's docstring, dense, differentiable in theta, z_all and obs_log_var by autograd."""
    L, T, a_lt, H = ref_whiten_diff(theta, z_all, prev, nu2, eps, dtype)
    Phi, c, sums = ref_moments_diff(theta, z_all, x, w, y, nu2, dtype)
    n_lt = a_lt.shape[-1]
    M = z_all.shape[-2] - n_lt
    A = T @ Phi @ T.mT
    tc = (T @ c.unsqueeze(-1)).squeeze(-1)
    sw, syy = sums[:, 0], sums[:, 1]
    beta = temper * (-obs_log_var.to(dtype)).exp()
    g2 = (2.0 * theta[-1].to(dtype)).exp()
    mv = lambda B, v: (B @ v.unsqueeze(-1)).squeeze(-1)
    b_t = tc[:, n_lt:] - mv(A[:, n_lt:, :n_lt], a_lt)
    Lb = torch.linalg.cholesky(torch.eye(M, dtype=dtype) + beta.view(-1, 1, 1) * A[:, n_lt:, n_lt:])
    quad = torch.linalg.solve_triangular(Lb, b_t.unsqueeze(-1), upper=False).square().sum((-2, -1))
    logdet = 2.0 * Lb.diagonal(dim1=-2, dim2=-1).log().sum(-1)
    trHAH, o = torch.zeros_like(sw), 0
    for H_i in H:
        n = H_i.shape[-1]
        trHAH = trHAH + (H_i * (A[:, o:o + n, o:o + n] @ H_i)).sum((-2, -1))
        o += n
    fixed = syy - 2.0 * (a_lt * tc[:, :n_lt]).sum(-1) + (a_lt * mv(A[:, :n_lt, :n_lt], a_lt)).sum(-1) + g2 * sw \
        - A.diagonal(dim1=-2, dim2=-1).sum(-1) + trHAH
    return -0.5 * sw * (2.0 * math.pi / beta).log() - 0.5 * beta * fixed + 0.5 * beta ** 2 * quad - 0.5 * logdet


def ref_bound_grads(theta, z_lt, z_t, prev, x, y, w, obs_log_var, nu2, temper=1.0, dtype=torch.float64):
    """-> (bound (C,), d sum(bound) / d (theta, z_t, obs_log_var)) with the frozen tasks' z_lt (C, n_<, D) a constant."""
    th, zt, olv = (t.detach().to(dtype).clone().requires_grad_(True) for t in (theta, z_t, obs_log_var))
    b = ref_bound(th, torch.cat([z_lt.to(dtype), zt], -2), prev, x, y, w, olv, nu2, temper=temper, dtype=dtype)
    return b.detach(), torch.autograd.grad(b.sum(), (th, zt, olv))


@pytest.mark.parametrize('nu2', [0, 3])
@pytest.mark.parametrize('t', [0, 2])
def test_restated_bound_is_ref_fits_and_its_gradient_is_the_central_difference(t, nu2):
    """M = 5, D = 3, N = 40, two outputs, weights, temper 0.7, fp64: the value is ref_fit's to 1e-11; every entry of autograd's
    gradient for (theta, z_t, obs_log_var) is the central difference (h = 1e-5: truncation ~ h^2, rounding ~ 1e-16 |bound| / h)
    to 1e-6 of the gradient's largest entry."""
    M = 5
    pr = make_problem(2, M, t, 3, 40, seed=20 + t, weights=True)
    z_lt, z_t = pr['z_all'][:, :t * M], pr['z_all'][:, t * M:]
    args = (pr['prev'], pr['x'], pr['y'], pr['w'])
    val, grads = ref_bound_grads(pr['theta'], z_lt, z_t, *args, pr['obs_log_var'], nu2, temper=0.7)
    fit = ref_fit(pr['theta'], pr['z_all'], *args, pr['obs_log_var'], nu2, temper=0.7)
    assert torch.allclose(val, fit['bound'], rtol=1e-11, atol=0.0)
    for u, v in zip(ref_whiten_diff(pr['theta'], pr['z_all'], pr['prev'], nu2)[:3], ref_whiten(pr['theta'], pr['z_all'], pr['prev'], nu2)[:3]):
        assert torch.allclose(u, v, rtol=1e-13, atol=1e-15)
    # the differentiable moments are ref_moments', in value and (away from coincident points) in autograd's gradient
    th = [pr['theta'].double().requires_grad_(True) for _ in range(2)]
    zz = [pr['z_all'].double().requires_grad_(True) for _ in range(2)]
    outs = [fn(th[k], zz[k], pr['x'], pr['w'], pr['y'], nu2) for k, fn in enumerate((ref_moments_diff, ref_moments))]
    assert all(torch.allclose(u, v, rtol=1e-14, atol=0.0) for u, v in zip(*outs))
    gs = [torch.autograd.grad(o[0].sin().sum() + o[1].cos().sum(), (th[k], zz[k])) for k, o in enumerate(outs)]
    assert all(torch.allclose(u, v, rtol=1e-12, atol=1e-14) for u, v in zip(*gs))
    base = [pr['theta'].double(), z_t.double(), pr['obs_log_var'].double()]
    f = lambda th, zt, olv: ref_bound(th, torch.cat([z_lt.double(), zt], -2), *args, olv, nu2, temper=0.7).sum().item()
    h = 1e-5
    for k, (p, g) in enumerate(zip(base, grads)):
        fd = torch.zeros_like(p)
        for e in range(p.numel()):
            hi, lo = [q.clone() for q in base], [q.clone() for q in base]
            hi[k].view(-1)[e] += h
            lo[k].view(-1)[e] -= h
            fd.view(-1)[e] = (f(*hi) - f(*lo)) / (2.0 * h)
        err = (fd - g).abs().max().item() / g.abs().max().item()
        print(f't={t} nu2={nu2} parameter {k}: |grad| {g.abs().max().item():.3e}, central-difference mismatch {err:.2e}')
        assert err < 1e-6, (t, nu2, k, err)


@pytest.mark.parametrize('nu2', [0, 1, 3, 5])
def test_log_gamma_gradient_needs_no_pass_over_the_data(nu2):
    """K = gamma^2 f(distances): d/d log gamma of <gPhi, Phi> + <gc, c> is 4 <gPhi, Phi> + 2 <gc, c> for ANY gPhi -- random and not
    symmetric here (fp64 autograd of ref_moments; what _GramMoments.backward writes into gtheta[D])."""
    g = torch.Generator().manual_seed(3 + nu2)
    G, Mt, N, D = 2, 7, 30, 3
    theta = (0.3 * torch.randn(D + 1, generator=g)).double().requires_grad_(True)
    Z, X = torch.randn(G, Mt, D, generator=g).double(), torch.randn(N, D, generator=g).double()
    w, y = torch.rand(G, N, generator=g).double(), torch.randn(G, N, generator=g).double()
    gPhi, gc = torch.randn(G, Mt, Mt, generator=g).double(), torch.randn(G, Mt, generator=g).double()
    assert not torch.equal(gPhi, gPhi.mT)
    Phi, c, _ = ref_moments(theta, Z, X, w, y, nu2)
    gth, = torch.autograd.grad((gPhi * Phi).sum() + (gc * c).sum(), theta)
    want = 4.0 * (gPhi * Phi.detach()).sum() + 2.0 * (gc * c.detach()).sum()
    assert abs(gth[-1].item() - want.item()) <= 1e-12 * abs(want.item())


# -- the C ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported():
    from vargp_amd import _lib
    for name in ('vargp_gram_moments_bwd', 'vargp_gram_moments_bwd_workspace_bytes', 'vargp_gram_moments_bwd_chunks'):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    L = _lib.lib()
    assert L.vargp_gram_moments_bwd.restype is ctypes.c_int and len(L.vargp_gram_moments_bwd.argtypes) == 17
    assert L.vargp_gram_moments_bwd_workspace_bytes.restype is ctypes.c_size_t
    assert L.vargp_gram_moments_bwd_chunks(1, 15, 1000, 3) > 1 and L.vargp_gram_moments_bwd_chunks(1, 15, 64, 3) == 1


def test_cabi_argument_errors_before_any_launch():
    """A null pointer other than w, a size < 1, a kernel code outside the four, G > 65535 or a short workspace: VARGP_EINVAL (-1)
    with host memory for pointers -- nothing is launched, so no device is touched."""
    from vargp_amd._lib import lib
    L = lib()
    EINVAL = -1
    G, Mt, N, D = 2, 5, 9, 3
    need = L.vargp_gram_moments_bwd_workspace_bytes(G, Mt, N, D)
    buf = (ctypes.c_float * (need // 4 + 16))()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)
    fn = L.vargp_gram_moments_bwd

    def call(ptrs=None, dims=(G, Mt, N, D), nu2=0, ws=p, ws_bytes=need):
        return fn(*(ptrs or [p] * 9), *dims, nu2, ws, ws_bytes, None)

    for bad in (0, 1, 2, 4, 5, 6, 7, 8):                             # every pointer but w (3)
        assert call([null if q == bad else p for q in range(9)]) == EINVAL
    assert call(ws=null) == EINVAL
    for dims in ((0, Mt, N, D), (G, 0, N, D), (G, Mt, 0, D), (G, Mt, N, 0), (-1, Mt, N, D), (65536, Mt, N, D)):
        assert call(dims=dims, ws_bytes=1 << 40) == EINVAL, dims
    for nu2 in (-1, 2, 4, 6):
        assert call(nu2=nu2) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and call(ws_bytes=0) == EINVAL
    assert b'gram_moments_bwd' in L.vargp_last_error()


def test_workspace_does_not_grow_with_the_data():
    """Per-chunk partials and S only.  Once the chunk count has saturated (the workgroup target binds: G x panels >= 512, or the
    byte budget of the partials of P binds) N = 1e3 and N = 1e7 need the same bytes; the partials of r and P never exceed the
    budget of 64 MiB unless one chunk alone does; at a fixed chunk count (N = 1000: four chunks) the bytes are non-decreasing in
    Mt and in D."""
    from vargp_amd._lib import lib
    ws, chunks = lib().vargp_gram_moments_bwd_workspace_bytes, lib().vargp_gram_moments_bwd_chunks
    for G, Mt, D in ((64, 512, 8), (600, 100, 2), (16, 2048, 784), (1024, 15, 40)):
        assert chunks(G, Mt, 1000, D) == chunks(G, Mt, 10 ** 7, D), (G, Mt, D)
        assert ws(G, Mt, 1000, D) == ws(G, Mt, 10 ** 7, D) > 0, (G, Mt, D)
    budget = 64 << 20
    for G, Mt, D in ((1, 100, 8), (1, 512, 8), (10, 100, 784), (3, 2048, 784), (1, 15, 2)):
        nt = (Mt + 63) // 64
        for N in (1, 1000, 10 ** 6, 2 * 10 ** 9):
            n = chunks(G, Mt, N, D)
            assert 1 <= n <= min(1024, (N + 255) // 256)
            assert n == 1 or n * G * nt * 64 * (D + 1) * 4 <= budget
            assert ws(G, Mt, N, D) <= n * G * nt * (64 * (D + 1) + D + 192) * 4 + G * (Mt * Mt + 64) * 4 + 1024
        big = [ws(G, Mt, N, D) for N in (10 ** 7, 10 ** 8, 2 * 10 ** 9)]
        assert max(big) <= 1.02 * min(big)                            # (the chunk length is rounded to 64 columns: not exactly equal)
    for D in (1, 8, 33, 784):
        sizes = [ws(1, Mt, 1000, D) for Mt in (1, 15, 64, 65, 130, 200, 512)]
        assert all(chunks(1, Mt, 1000, D) == 4 for Mt in (1, 15, 64, 65, 130, 200, 512))
        assert sizes == sorted(sizes), (D, sizes)
    for Mt in (15, 130, 512):
        sizes = [ws(1, Mt, 1000, D) for D in (1, 2, 32, 33, 64, 65, 129, 784)]
        assert sizes == sorted(sizes), (Mt, sizes)
    assert ws(0, 5, 5, 5) == 0 and chunks(1, 0, 5, 5) == 0


# -- the Python surface -------------------------------------------------------------------------------------------------------------
def test_the_bound_names_what_it_refuses():
    from vargp_amd._lib import VargpHipError
    from vargp_amd.kernels import DeepRBFKernel
    from vargp_amd.likelihoods import GaussianLikelihood
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 3, generator=g)
    reg = _Data(x, x[:, 0].clone())
    deep = VARGP(torch.randn(1, 4, 3, generator=g), DeepRBFKernel(3, feature_size=6), GaussianLikelihood(1))
    for call in (lambda gp, *a: gp.collapsed_bound(*a), lambda gp, *a: gp.fit_collapsed_(*a, n_steps=1)):
        with pytest.raises(ValueError, match='DeepRBFKernel'):
            call(deep, x, reg.targets)
        with pytest.raises(ValueError, match='GaussianLikelihood'):
            call(VARGP.create_clf(_Data(x, torch.arange(40) % 3), M=4), x, torch.arange(40) % 3)
        with pytest.raises(ValueError, match='GaussianLikelihood'):
            call(VARGP.create_reg(reg, M=4, likelihood='studentt'), x, reg.targets)
        with pytest.raises(ValueError, match='ep_var_mean=True'):
            call(VARGP.create_reg(reg, M=4, ep_var_mean=False), x, reg.targets)
        with pytest.raises(VargpHipError):                          # a supported model on the host: no CPU path
            call(VARGP.create_reg(reg, M=4), x, reg.targets)
        with pytest.raises(VargpHipError):
            call(VARGP.create_reg(reg, M=4, kernel='matern32'), x, reg.targets)
    with pytest.raises(ValueError, match='params'):
        VARGP.create_reg(reg, M=4).fit_collapsed_(x, reg.targets, params=('z', 'q'))
    with pytest.raises(ValueError, match='gaussian'):
        VARGP.create_reg(reg, M=4, likelihood='poisson', q_init='collapsed')
    with pytest.raises(ValueError, match='q_init'):
        VARGP.create_reg(reg, M=4, q_init='sgpr')


def test_gram_moments_diff_refuses_what_it_cannot_differentiate():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    theta, Z, X, y = torch.zeros(4), torch.randn(1, 5, 3), torch.randn(9, 3), torch.randn(1, 9)
    for name, kw in (('X', dict(X=X.clone().requires_grad_(True))), ('y', dict(y=y.clone().requires_grad_(True))),
                     ('w', dict(w=torch.rand(1, 9).requires_grad_(True)))):
        args = dict(theta=theta, Z=Z, X=X, w=None, y=y)
        args.update(kw)
        with pytest.raises(ValueError, match=f'{name} requires grad'):
            ops.gram_moments_diff(**args)
    with pytest.raises(VargpHipError):
        ops.gram_moments_diff(theta.requires_grad_(True), Z, X, None, y)


# -- the toy problem of the device's fit_collapsed_ test -----------------------------------------------------------------------------
TOY_LENGTHSCALE, TOY_START = 0.5, 10.0             # the scale of the function's wiggles; the start is TOY_START times too long
TOY_KERNEL, TOY_NU2 = 'matern12', 1                # K(z, z) of ten points within one RBF (or Matern-3/2) lengthscale is beyond the fp32
                                                   # whitening of fit_q_ (I + beta A_tt comes out indefinite at step 0); Matern-1/2's is not


def toy_regression(N=400, n_test=100, seed=0):
    """1-D: y = sin(3 x) + 0.1 noise on x ~ U(-2.5, 2.5).  -> x (N, 1), y (N,), xs (n_test, 1), ys (n_test,), float32."""
    g = torch.Generator().manual_seed(seed)
    x = 5.0 * torch.rand(N + n_test, 1, generator=g) - 2.5
    y = torch.sin(3.0 * x[:, 0]) + 0.1 * torch.randn(N + n_test, generator=g)
    return x[:N], y[:N], x[N:], y[N:]


def ref_heldout_logprob(theta, z, x, y, xs, ys, olv, nu2=TOY_NU2):
    """per held-out point, log N(ys | mu, var + sigma^2) of the model fitted by ref_fit at (theta, z, olv), fp64."""
    fit = ref_fit(theta, z, [], x, y.unsqueeze(0), None, olv, nu2)
    mu, var = ref_predict(theta, z, [fit['u_mean'].unsqueeze(-1)], [fit['u_tril']], xs, nu2)
    tot = var[0] + olv.double().exp()
    return -0.5 * (2.0 * math.pi * tot).log() - 0.5 * (ys.double() - mu[0]) ** 2 / tot


def test_the_toy_start_leaves_a_clear_gain_to_ascent_on_the_bound():
    """N = 400, M = 10, Matern-1/2, the lengthscale 10 times too long, obs_log_var = -4 as GaussianLikelihood starts: 60 steps of plain
    gradient ascent (a step of 0.05 along the gradient scaled to unit largest entry, per parameter) on the fp64 restatement
    raise the bound by more than 1 nat per training point (each point, on average, more than e times as probable under the
    bound), and the held-out log density of 100 points by more than three standard errors of the paired per-point differences
    (a gain that is not sampling noise of the held-out set) -- the conditions under which tests/test_hip_collapsed_grad.py
    expects fit_collapsed_ to beat fit_q_ alone."""
    x, y, xs, ys = toy_regression()
    g = torch.Generator().manual_seed(1)
    z = x[torch.randperm(400, generator=g)[:10]].unsqueeze(0).double()
    theta = torch.tensor([math.log(TOY_START * TOY_LENGTHSCALE), 0.0], dtype=torch.float64)
    olv = torch.tensor([-4.0], dtype=torch.float64)
    before = ref_heldout_logprob(theta, z, x, y, xs, ys, olv)
    params = [theta.clone().requires_grad_(True), z.clone().requires_grad_(True), olv.clone().requires_grad_(True)]
    trace = []
    for _ in range(60):
        b = ref_bound(params[0], params[1], [], x, y.unsqueeze(0), None, params[2], TOY_NU2).sum()
        trace.append(b.item())
        grads = torch.autograd.grad(b, params)
        with torch.no_grad():
            for p, gr in zip(params, grads):
                p += 0.05 * gr / gr.abs().max().clamp_min(1e-300)
    trace.append(ref_bound(params[0], params[1], [], x, y.unsqueeze(0), None, params[2], TOY_NU2).sum().item())
    after = ref_heldout_logprob(*[p.detach() for p in params[:2]], x, y, xs, ys, params[2].detach())
    diff = after - before
    gain, se = diff.sum().item(), math.sqrt(diff.numel()) * diff.std().item()
    print(f'bound {trace[0]:.1f} -> {trace[-1]:.1f}; held-out log density {before.sum().item():.1f} -> {after.sum().item():.1f} '
          f'(gain {gain:.1f}, standard error {se:.1f}); lengthscale '
          f'{params[0][0].exp().item():.3f}, noise variance {params[2].exp().item():.4f}')
    assert all(math.isfinite(v) for v in trace)
    assert trace[-1] - trace[0] > 1.0 * 400 and gain > 3.0 * se
