"""GPU: the Matern kernel (nu = 1/2, 3/2, 5/2) -- vargp_matern_gram_{fwd,bwd}, ops.matern_gram, kernels.MaternKernel -- and, at
op level (section a and b), the RBF op built on the same frame (csrc/gram.hip): vargp_rbf_gram_{fwd,bwd}, ops.rbf_gram, as the
kernel 'rbf' of the same matrix, K / gamma^2 = exp(-d2 / 2).

The reference has no Matern kernel, so the yardstick is `matern_ref` below: an fp64 torch restatement of

    d2 = sum_k ((x_k - y_k) / l_k)^2,  r = sqrt(max(d2, 0)),
    K / gamma^2 = exp(-r) | (1 + sqrt3 r) exp(-sqrt3 r) | (1 + sqrt5 r + 5 r^2 / 3) exp(-sqrt5 r),

differentiated by autograd, with the derivative of nu = 1/2 with respect to d2 DEFINED as 0 where d2 <= 0.  The same function
in fp32 on one host thread gives the floor of the project's parity rule (tests/sweep_rule.py), per class of quantities:

    err(HIP, fp64) <= tol + 2 x err(fp32 restatement, fp64),   tol = RTOL_SCALAR (K by relative L2, the ELBO scalars) or
                                                               REL_L2_GRAD (gradients by relative L2), tests/helpers.py.

Model level: the pinned oracle algorithm (oracle/vargp_oracle.py) with only its module-level `rbf_gram` swapped for
`matern_ref` (monkeypatch, undone after each test).
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import ATOL_PRED, REL_L2_GRAD, RTOL_PRED, RTOL_SCALAR, rel_l2, to_dev

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DIRECT_D = 32                      # csrc/common.h kRbfDirectD: D <= this takes the direct distance form, above it the GEMM
NUS = (0.5, 1.5, 2.5)
RBF = 'rbf'
KERNELS = (RBF,) + NUS             # the op-level matrix: `nu` is RBF or a Matern nu
EPS32 = float(np.finfo(np.float32).eps)


class _Sqrt0(torch.autograd.Function):
    """sqrt with the convention of the issue: d sqrt(d2) / d d2 = 0 where d2 <= 0."""
    @staticmethod
    def forward(ctx, d2):
        r = d2.clamp_min(0).sqrt()
        ctx.save_for_backward(r)
        return r

    @staticmethod
    def backward(ctx, g):
        r, = ctx.saved_tensors
        return torch.where(r > 0, g / (2 * r.clamp_min(1e-300 if r.dtype == torch.float64 else 1e-30)), torch.zeros_like(g))


def _k_of_d2(d2, nu):
    if nu == RBF:
        return (-0.5 * d2).exp()
    d2 = d2.clamp_min(0)
    if nu == 0.5:
        return (-_Sqrt0.apply(d2)).exp()
    # closed forms in d2 whose autograd derivative is finite at 0: d/dd2 [(1 + a) e^-a], a = sqrt(c d2), is -(c/2) e^-a.
    # sqrt(d2 + 0) at d2 = 0 has an infinite autograd derivative, so r enters through _Sqrt0 and the exact d2-derivative is
    # restored by a custom node
    return _KSmooth.apply(d2, nu)


class _KSmooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d2, nu):
        c = 2 * nu
        a = (c * d2).sqrt()
        e = (-a).exp()
        ctx.save_for_backward(a, e)
        ctx.nu = nu
        return (1 + a) * e if nu == 1.5 else (1 + a + (5.0 / 3.0) * d2) * e

    @staticmethod
    def backward(ctx, g):
        a, e = ctx.saved_tensors
        dk = -1.5 * e if ctx.nu == 1.5 else -(5.0 / 6.0) * (1 + a) * e
        return g * dk, None


def matern_ref(theta, x, y=None, full_gram=False, nu=2.5):
    """Signature of oracle.rbf_gram: theta (S, D+1); x (..., M, D); y (..., N, D) or None -> (S, ..., M, N).  The distance is
    formed directly (differences), in the dtype of the inputs."""
    S = theta.shape[0]
    lead = x.dim() - 2
    th = theta.reshape(S, *([1] * lead), 1, -1)
    sig = th[..., :-1].exp()
    g2 = (2.0 * th[..., -1:]).exp()
    a = x.unsqueeze(0) / sig
    b = a if y is None else y.unsqueeze(0) / sig
    d2 = ((a.unsqueeze(-2) - b.unsqueeze(-3)) ** 2).sum(-1)
    return g2 * _k_of_d2(d2, nu)


def _one_thread(fn):
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(n)


# -- a. op level ------------------------------------------------------------------------------------------------------------------
def _op_inputs(S, C, M, N, D, mode, seed):
    """Well-separated uniform points; log lengthscales near log 0.5 (D = 784: x 0.15 data, lengthscales near
    log(0.5 sqrt(D) 0.15)), so that K is O(0.1 .. 1) at every D."""
    gen = torch.Generator().manual_seed(seed)
    scale = 0.15 if D >= 256 else 1.0
    ell = 0.5 * math.sqrt(D) * scale if D > 2 else 0.5
    theta = torch.cat([math.log(ell) + 0.1 * torch.randn(S, D, generator=gen),
                       math.log(0.7) + 0.1 * torch.randn(S, 1, generator=gen)], dim=1)
    X = scale * torch.rand(C, M, D, generator=gen)
    Y = None if mode == 'self' else scale * torch.rand(*((N, D) if mode == 'shared' else (C, N, D)), generator=gen)
    gK = torch.randn(S, C, M, M if mode == 'self' else N, generator=gen)
    return theta, X, Y, gK


def _ref_op(theta, X, Y, gK, nu, dtype):
    th, x = theta.to(dtype).requires_grad_(True), X.to(dtype).requires_grad_(True)
    y = None if Y is None else Y.to(dtype).requires_grad_(True)
    yy = None if y is None else (y.unsqueeze(0).expand(X.shape[0], -1, -1) if y.dim() == 2 else y)
    K = matern_ref(th, x, yy, nu=nu)
    gs = torch.autograd.grad((K * gK.to(dtype)).sum(), [th, x] + ([] if y is None else [y]))
    out = dict(K=K.detach(), gtheta=gs[0], gX=gs[1])
    if y is not None:
        out['gY'] = gs[2]
    return out


def _hip_op(theta, X, Y, gK, nu, shared):
    from vargp_amd import ops
    th, x = theta.to(DEV).requires_grad_(True), X.to(DEV).requires_grad_(True)
    y = None if Y is None else Y.to(DEV).requires_grad_(True)
    K = ops.rbf_gram(th, x, y, shared) if nu == RBF else ops.matern_gram(th, x, y, shared, nu)
    gs = torch.autograd.grad(K, [th, x] + ([] if y is None else [y]), gK.to(DEV))
    torch.cuda.synchronize()
    out = dict(K=K.detach().cpu(), gtheta=gs[0].cpu(), gX=gs[1].cpu())
    if y is not None:
        out['gY'] = gs[2].cpu()
    return out


def _check_rule(got, r32, r64, tag):
    """K on its own (tol RTOL_SCALAR); the gradients as one class (tol REL_L2_GRAD, floor: the worst of the class)."""
    errs = {k: (rel_l2(got[k], r64[k]), rel_l2(r32[k], r64[k])) for k in r64}
    print(tag, {k: ('%.2e' % a, '%.2e' % b) for k, (a, b) in errs.items()}, flush=True)
    assert errs['K'][0] <= RTOL_SCALAR + 2.0 * errs['K'][1], (tag, 'K', errs['K'])
    floor = max(b for k, (_, b) in errs.items() if k != 'K')
    for k, (a, _) in errs.items():
        if k != 'K':
            assert a <= REL_L2_GRAD + 2.0 * floor, (tag, k, a, floor)


def _run_op_case(S, C, M, N, D, mode, nu, seed):
    theta, X, Y, gK = _op_inputs(S, C, M, N, D, mode, seed)
    r64 = _ref_op(theta, X, Y, gK, nu, torch.float64)
    r32 = _one_thread(lambda: _ref_op(theta, X, Y, gK, nu, torch.float32))
    got = _hip_op(theta, X, Y, gK, nu, mode == 'shared')
    _check_rule(got, r32, r64, f'nu={nu} {mode} S{S} C{C} M{M} N{N} D{D}')
    if mode == 'self':             # exact gamma^2 diagonal (tests/test_hip_ops.py: test_rbf_gram_fwd_bwd)
        g2 = torch.exp(2 * theta.to(DEV)[:, -1]).cpu()
        assert torch.equal(got['K'].diagonal(dim1=-2, dim2=-1), g2.view(-1, 1, 1).expand(S, C, M))


@pytest.mark.parametrize('nu', KERNELS)
@pytest.mark.parametrize('mode', ['self', 'batched', 'shared'])
@pytest.mark.parametrize('D', [1, 2, DIRECT_D, DIRECT_D + 1, 36, 784])
def test_op_vs_fp64_over_D(nu, mode, D):
    """Both sides of the direct / GEMM switch (33 is no multiple of 4: scalar operand loads; 36 is: vector loads), D = 784."""
    _run_op_case(2, 3, 40, 72, D, mode, nu, seed=100 + D)


@pytest.mark.parametrize('nu', KERNELS)
@pytest.mark.parametrize('mode', ['self', 'batched', 'shared'])
@pytest.mark.parametrize('M,N', [(1, 1), (63, 65), (64, 64), (65, 63), (100, 257), (257, 100)])
def test_op_vs_fp64_edge_sizes(nu, mode, M, N):
    """Tile edges of the distance GEMM (D = 40) and of the W / finalisation kernels."""
    _run_op_case(2, 2, M, N, 40, mode, nu, seed=7 * M + N)


@pytest.mark.parametrize('nu', KERNELS)
@pytest.mark.parametrize('mode', ['self', 'batched', 'shared'])
@pytest.mark.parametrize('tile', [1, 2, 3])
def test_op_vs_fp64_every_gemm_tile(nu, mode, tile):
    """The 128 x 128 x 16 and 128 x 64 x 32 tiles are chosen for problems too large for an fp64 restatement on the host:
    force each tile shape (vargp_tune_gemm_tile) on a case with interior and edge tiles; D = 33 / 36: scalar / vector loads."""
    from vargp_amd._lib import lib
    try:
        assert lib().vargp_tune_gemm_tile(tile) == 0
        for D in (33, 36):
            _run_op_case(2, 2, 150, 200, D, mode, nu, seed=tile + D)
    finally:
        lib().vargp_tune_gemm_tile(0)


@pytest.mark.parametrize('nu', KERNELS)
@pytest.mark.parametrize('D', [2, 40])
def test_op_edge_sizes_direct_and_accumulate(nu, D):
    """accumulate = 1 of the C entry: a second backward adds into gX / gY / gtheta."""
    from vargp_amd._lib import lib, ptr, check, scratch, stream_ptr
    S, C, M, N = 2, 3, 65, 100
    theta, X, Y, gK = _op_inputs(S, C, M, N, D, 'batched', 5 + D)
    r64 = _ref_op(theta, X, Y, gK, nu, torch.float64)
    r32 = _one_thread(lambda: _ref_op(theta, X, Y, gK, nu, torch.float32))
    th, x, y, g = (t.to(DEV).contiguous() for t in (theta, X, Y, gK))
    if nu == RBF:                  # (its forward and backward workspaces are laid out differently: the larger of the two)
        ws_bytes, fwd, bwd, kind = lib().vargp_rbf_workspace_bytes, lib().vargp_rbf_gram_fwd, lib().vargp_rbf_gram_bwd, (0,)
    else:
        ws_bytes, fwd, bwd = lib().vargp_matern_workspace_bytes, lib().vargp_matern_gram_fwd, lib().vargp_matern_gram_bwd
        kind = (0, int(round(2 * nu)))                                    # y_shared, nu2
    K = torch.empty(S, C, M, N, device=DEV)
    ws = scratch(max(ws_bytes(S, C, M, N, D, 0), ws_bytes(S, C, M, N, D, 1)), torch.device(DEV))
    check(fwd(ptr(th), ptr(x), ptr(y), ptr(K), S, C, M, N, D, *kind, ptr(ws), ws.numel() * 4, stream_ptr()), 'fwd')
    base = dict(gX=torch.randn(C, M, D), gY=torch.randn(C, N, D), gtheta=torch.randn(S, D + 1))
    out = {k: v.to(DEV).clone() for k, v in base.items()}
    check(bwd(ptr(th), ptr(x), ptr(y), ptr(K), ptr(g), ptr(out['gX']), ptr(out['gY']), ptr(out['gtheta']), S, C, M, N, D,
              *kind, 1, ptr(ws), ws.numel() * 4, stream_ptr()), 'bwd')
    torch.cuda.synchronize()
    got = {k: out[k].cpu() - base[k] for k in base}
    got['K'] = K.cpu()
    _check_rule(got, r32, r64, f'accumulate nu={nu} D{D}')


def test_bad_nu_is_an_error():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError, lib, ptr, check, scratch, stream_ptr
    th, x = torch.zeros(1, 3, device=DEV), torch.zeros(1, 4, 2, device=DEV)
    with pytest.raises(ValueError):
        ops.matern_gram(th, x, nu=2.0)
    K = torch.empty(1, 1, 4, 4, device=DEV)
    ws = scratch(lib().vargp_matern_workspace_bytes(1, 1, 4, 4, 2, 1), torch.device(DEV))
    for nu2 in (0, 2, 7):
        with pytest.raises(VargpHipError):
            check(lib().vargp_matern_gram_fwd(ptr(th), ptr(x), None, ptr(K), 1, 1, 4, 4, 2, 0, nu2, ptr(ws), ws.numel() * 4,
                                              stream_ptr()), 'fwd')


_SPLITK_SCRIPT = '''
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_hip_matern as t
for nu in t.KERNELS:
    for mode in ('self', 'batched', 'shared'):
        t._run_op_case(2, 3, 70, 130, 784, mode, nu, seed=11)
print('splitk ok')
'''


def test_op_vs_fp64_split_k():
    """The K-split distance product (partial inner products + combine pass) is off by default and chosen once per process
    (VARGP_RBF_SPLITK): the same op cases in a fresh interpreter with two splits."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, VARGP_RBF_SPLITK='2')
    r = subprocess.run([sys.executable, '-c', _SPLITK_SCRIPT % (os.path.dirname(here), here)], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0 and 'splitk ok' in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# -- b. r = 0 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nu', KERNELS)
@pytest.mark.parametrize('D', [2, 40])
@pytest.mark.parametrize('copy', [False, True])
def test_coincident_points(nu, D, copy):
    """Y = NULL (the diagonal is gamma^2 by construction) and Y a copy of X (the diagonal distance comes out of the arithmetic:
    exactly 0 in the direct form, D <= 32; rounding noise of the inner-product form above, clamped at 0).
    Bound for the copy's diagonal, D > 32: d2 = na + nb - 2 ab with three fp32 dot products of D terms, each within
    D eps |a|^2 of its value (worst-case summation), so |d2| <= 4 D eps na, and 1 - k(r) <= sqrt(2 nu) r for every nu here.
    The RBF does not clamp d2: |1 - exp(-d2 / 2)| <= t exp(t) with t = |d2| / 2 <= 2 D eps na."""
    S, C, M = 2, 2, 50
    theta, X, _, gK = _op_inputs(S, C, M, M, D, 'self', 31 + D)
    Y = X.clone() if copy else None
    got = _hip_op(theta, X, Y, gK, nu, False)
    g2 = (2.0 * theta[:, -1].double()).exp().float()                      # the kernel's own g2 = expf(2 theta_D) to fp32 rounding
    diag = got['K'].diagonal(dim1=-2, dim2=-1)                            # (S, C, M)
    if not copy or D <= DIRECT_D:
        hip_g2 = diag[:, 0, 0]
        assert torch.equal(diag, hip_g2.view(S, 1, 1).expand_as(diag))   # one value per hyper-sample, bit for bit
        np.testing.assert_allclose(hip_g2.numpy(), g2.numpy(), rtol=4 * EPS32)
    else:
        na = ((X.double().unsqueeze(0) / theta[:, :-1].double().exp().view(S, 1, 1, D)) ** 2).sum(-1)      # (S, C, M)
        t = 2 * D * EPS32 * na
        bound = (t * t.exp() if nu == RBF else (2 * nu * 4 * D * EPS32 * na).sqrt()) + 4 * EPS32
        dev = (1.0 - diag.double() / g2.double().view(S, 1, 1)).abs()
        print('copy diagonal: worst deviation %.2e, bound there %.2e' % (dev.max().item(), bound.flatten()[dev.argmax()].item()))
        assert (dev <= bound).all()
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    # against the restatement with the same convention (for nu = 1/2: nothing from the coincident pairs)
    r64 = _ref_op(theta, X, Y, gK, nu, torch.float64)
    r32 = _one_thread(lambda: _ref_op(theta, X, Y, gK, nu, torch.float32))
    if copy and D > DIRECT_D and nu == 0.5:
        # the inner-product form's diagonal of K is sqrt(noise) away from gamma^2 (bounded above): compare K off the diagonal
        off = ~torch.eye(M, dtype=torch.bool)
        for r in (got, r32, r64):
            r['K'] = r['K'][..., off]
    _check_rule(got, r32, r64, f'r=0 nu={nu} D{D} copy={int(copy)}')
    if nu == 0.5 and not copy:
        # only the diagonal's gK differs, by 1000 where the rest is O(1): gX must not move at all; the lengthscale part of
        # gtheta is summed with float atomics, whose order varies from run to run, so it may move by that rounding (a few
        # eps32 of its norm; 64 eps32 allows for sums of some hundred terms) and no more
        gK2 = gK + torch.eye(M) * 1000.0
        got2 = _hip_op(theta, X, Y, gK2, nu, False)
        assert torch.equal(got2['gX'], got['gX'])
        assert rel_l2(got2['gtheta'][:, :D], got['gtheta'][:, :D]) <= 64 * EPS32


# -- c. model level ---------------------------------------------------------------------------------------------------------------
def _dbl(t):
    if isinstance(t, torch.Tensor):
        return t.double() if t.is_floating_point() else t
    if isinstance(t, dict):
        return {k: _dbl(v) for k, v in t.items()}
    if isinstance(t, (list, tuple)):
        return type(t)(_dbl(v) for v in t)
    return t


def _build(params, prev, S, nu, lik, ep_var_mean=True, cls=None):
    from vargp_amd.kernels import MaternKernel
    from vargp_amd.vargp import VARGP
    D = params['z'].shape[-1]
    kern = MaternKernel(D, nu=nu, prior_log_mean=params['prior_log_mean'], prior_log_logvar=params['prior_log_logvar'])
    kw = {} if cls is not None else dict(ep_var_mean=ep_var_mean)
    gp = (cls or VARGP)(params['z'], kern, lik, n_var_samples=S, prev_params=[{k: v.clone() for k, v in p.items()} for p in prev],
                        **kw)
    with torch.no_grad():
        gp.kernel.log_mean.copy_(params['log_mean'])
        gp.kernel.log_logvar.copy_(params['log_logvar'])
        gp.u_mean.copy_(params['u_mean'])
        gp.u_tril_vec.copy_(params['u_tril_vec'])
    return gp.to(DEV)


def _no_native_program(gp):
    progs = (gp._t0_progs, gp._t0_spares, gp._tn_progs, gp._tn_spares)
    assert not any(progs), f'a Matern model created a native program: {progs}'


NAMES = ['z', 'u_mean', 'u_tril_vec', 'log_mean', 'log_logvar']
BETA, NTOT = 2.0, 7.0


def _oracle_gauss(params, prev, x, y, nz, olv, ep_var_mean):
    """orc.elbo_step with the Gaussian expected log-likelihood (tests/test_hip_gauss.py: _fp64) in place of softmax_nll."""
    leaf = dict(params)
    for k in NAMES:
        leaf[k] = params[k].detach().clone().requires_grad_(True)
    lo = olv.to(params['z'].dtype).requires_grad_(True)
    pmu, pvar, (mu_q, Lq, mu_p, Lp) = orc.forward(leaf, prev, x, nz, want_kl=True, ep_var_mean=ep_var_mean)
    kl_u = orc.mvn_kl(mu_q, Lq, mu_p, Lp).sum(-1).mean(0).mean(0)
    kl_h = orc.kl_hypers(leaf['log_mean'], leaf['log_logvar'], leaf['prior_log_mean'], leaf['prior_log_logvar'])
    nll = -torch.distributions.Normal(pmu, (pvar + lo.exp().view(1, -1, 1)).sqrt()).log_prob(y.unsqueeze(0)).mean(0).mean(0).sum(0)
    total = BETA * kl_h + kl_u + NTOT * nll
    g = torch.autograd.grad(total, [leaf[k] for k in NAMES] + [lo])
    return dict(kl_hypers=kl_h.detach(), kl_u=kl_u.detach(), nll=nll.detach()), dict(zip(NAMES + ['obs_log_var'], g))


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('n_prev', [0, 1])
@pytest.mark.parametrize('nomean', [False, True])
@pytest.mark.parametrize('lik', ['softmax', 'gauss'])
@pytest.mark.parametrize('D', [2, 40])
def test_model_loss_and_grads_vs_oracle_with_matern(nu, n_prev, nomean, lik, D, monkeypatch):
    from vargp_amd import noise
    from vargp_amd.likelihoods import GaussianLikelihood, MulticlassSoftmax
    monkeypatch.setattr(orc, 'rbf_gram', lambda theta, x, y=None, full_gram=False: matern_ref(theta, x, y, nu=nu))
    S, F_, C, M, B = 2, 3, 3, 12, 48
    seed = 3 + int(2 * nu) + 10 * n_prev + D
    params, prev, x, y, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=n_prev, seed=seed, kind='wtoy' if D == 2 else 'gauss')
    if n_prev:                     # prev_params as a first Matern task leaves them: z, u_mean, u_tril_vec of its state dict
        first = _build(dict(params, **prev[0]), [], S, nu, MulticlassSoftmax(n_f=F_))
        prev = [{k: v.detach().cpu().clone() for k, v in first.state_dict().items() if k in ('z', 'u_mean', 'u_tril_vec')}]
    if lik == 'gauss':
        nz = {k: v for k, v in nz.items() if k != 'eps_f'}
        y = torch.sin(3.0 * x.sum(-1, keepdim=True).T + torch.arange(C).view(C, 1)).float()          # (C, B) targets
        olv = torch.linspace(-2.0, -1.0, C)
        run = lambda p, pv, xx, yy, n: _oracle_gauss(p, pv, xx, yy, n, olv, not nomean)
    else:
        run = lambda p, pv, xx, yy, n: orc.elbo_step(p, pv, xx, yy, n, beta=BETA, n_total=NTOT * B, ep_var_mean=not nomean)
    s64, g64 = run(_dbl(params), _dbl(prev), _dbl(x), _dbl(y), _dbl(nz))
    s32, g32 = _one_thread(lambda: run(params, prev, x, y, nz))

    gp = _build(params, prev, S, nu, GaussianLikelihood(C) if lik == 'gauss' else MulticlassSoftmax(n_f=F_), not nomean)
    if lik == 'gauss':
        with torch.no_grad():
            gp.likelihood.obs_log_var.copy_(olv)
    with noise.inject(**to_dev(nz, DEV)):
        kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
        (BETA * kl_h + kl_u + NTOT * nll).backward()
    _no_native_program(gp)
    sc = dict(kl_hypers=kl_h.item(), kl_u=kl_u.item(), nll=nll.item())
    gr = dict(z=gp.z.grad, u_mean=gp.u_mean.grad, u_tril_vec=gp.u_tril_vec.grad, log_mean=gp.kernel.log_mean.grad,
              log_logvar=gp.kernel.log_logvar.grad)
    if lik == 'gauss':
        gr['obs_log_var'] = gp.likelihood.obs_log_var.grad
    rel = lambda a, b: abs(a - b) / abs(b)
    e_sc = {k: (rel(v, s64[k].item()), rel(s32[k].item(), s64[k].item())) for k, v in sc.items() if s64[k].item() != 0.0}
    e_gr = {k: (rel_l2(g.cpu(), g64[k]), rel_l2(g32[k], g64[k])) for k, g in gr.items()}
    print({k: ('%.2e' % a, '%.2e' % b) for k, (a, b) in {**e_sc, **e_gr}.items()}, flush=True)
    for errs, tol in ((e_sc, RTOL_SCALAR), (e_gr, REL_L2_GRAD)):
        bound = tol + 2.0 * max(b for _, b in errs.values())
        for k, (a, _) in errs.items():
            assert a <= bound, (k, a, bound)


# -- d. trainer and driver ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nu', NUS)
def test_trainer_eager_and_captured_steps_agree(nu):
    from vargp_amd import noise, ops
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.train import ElboTrainer
    S, F_, C, M, D, B = 2, 2, 3, 16, 40, 64
    params, prev, x, y, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=0, seed=9, kind='gauss')
    xd, yd = x.to(DEV), y.to(DEV)
    ops.set_cholesky_error_mode('defer')
    ops.reset_linalg_errors()
    try:
        results = []
        for mode in ('graph', 'eager'):
            gp = _build(params, prev, S, nu, MulticlassSoftmax(n_f=F_))
            tr = ElboTrainer(gp, lr=1e-3, beta=2.0, n_total=10 * B)
            with noise.inject(**to_dev(nz, DEV)):
                if mode == 'graph':
                    tr.capture(xd, yd, warmup=1)
                    for _ in range(3):
                        out = tr.step_graph()
                else:
                    for _ in range(3):
                        out = tr.step(xd, yd)
            torch.cuda.synchronize()
            _no_native_program(gp)
            results.append(({k: v.detach().cpu().clone() for k, v in gp.state_dict().items()}, [float(o) for o in out]))
        (sd_g, out_g), (sd_e, out_e) = results
        np.testing.assert_allclose(out_g, out_e, rtol=1e-5)
        for k in sd_e:
            assert rel_l2(sd_g[k], sd_e[k]) < 1e-5, k
        assert ops.linalg_error_count() == 0
    finally:
        ops.set_cholesky_error_mode('raise')


@pytest.mark.parametrize('nu', NUS)
def test_toy_run_decreases_the_loss(nu):
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.train import ElboTrainer
    S, F_, C, M, D, B = 2, 4, 4, 12, 2, 128
    params, prev, x, _, _ = orc.make_problem(S, F_, C, M, D, B, n_prev=0, seed=21, kind='wtoy')
    y = ((x[:, 0] > 0).long() + 2 * (x[:, 1] > 0).long())                   # the quadrant: learnable from 2-D inputs
    gp = _build(params, prev, S, nu, MulticlassSoftmax(n_f=F_))
    tr = ElboTrainer(gp, lr=1e-2, beta=1.0, n_total=B)
    xd, yd = x.to(DEV), y.to(DEV)
    torch.manual_seed(0)
    totals = []
    for _ in range(200):
        kl_h, kl_u, nll = (float(v) for v in tr.step(xd, yd))
        totals.append(kl_h + kl_u + nll)
    _no_native_program(gp)
    first, last = np.mean(totals[:10]), np.mean(totals[-10:])
    print('toy run nu=%s: loss %.4f -> %.4f' % (nu, first, last))
    assert np.isfinite(totals).all() and last < first


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('n_prev,D', [(0, 8), (1, 40)])
def test_tiled_predict_equals_untiled(nu, n_prev, D):
    """One injected eps_theta; a GaussianLikelihood model, whose prediction (the predictive means, (S, C, B)) draws nothing else."""
    from vargp_amd import noise
    from vargp_amd.likelihoods import GaussianLikelihood
    S, C, M, B = 2, 3, 12, 100
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=41 + n_prev, kind='gauss')
    gp = _build(params, prev, S, nu, GaussianLikelihood(C))
    xd = x.to(DEV)
    with noise.inject(eps_theta=nz['eps_theta'].to(DEV)), torch.no_grad():
        one = gp.predict(xd)
        tiled = gp.predict(xd, tile=32)
    _no_native_program(gp)
    assert one.shape == (S, C, B) and tiled.shape == (S, C, B)
    np.testing.assert_allclose(tiled.cpu().numpy(), one.cpu().numpy(), rtol=RTOL_PRED, atol=ATOL_PRED)


def test_create_clf_builds_matern_and_hands_the_prior_over():
    from vargp_amd.kernels import MaternKernel
    from vargp_amd.datasets import ToyDataset
    from vargp_amd.vargp import VARGP
    ds = ToyDataset()
    gp0 = VARGP.create_clf(ds, M=6, n_f=3, n_var_samples=2, kernel='matern32').to(DEV)
    assert type(gp0.kernel) is MaternKernel and gp0.kernel.nu == 1.5
    xb, yb = (t.to(DEV) for t in ds[torch.arange(32)])
    sum(gp0.loss(xb, yb)).backward()
    _no_native_program(gp0)
    sd = {k: v.detach().clone() for k, v in gp0.state_dict().items()}
    gp1 = VARGP.create_clf(ds, M=6, n_f=3, n_var_samples=2, prev_params=[sd], kernel='matern32').to(DEV)
    assert type(gp1.kernel) is MaternKernel
    assert torch.equal(gp1.kernel.prior_log_mean.cpu(), gp0.kernel.log_mean.detach().cpu())
    assert torch.equal(gp1.kernel.prior_log_logvar.cpu(), gp0.kernel.log_logvar.detach().cpu())
    out = gp1.loss(xb, yb)
    sum(out).backward()
    assert all(torch.isfinite(v) for v in out)
    _no_native_program(gp1)


@pytest.mark.parametrize('nu', NUS)
def test_retrain_accepts_a_matern_kernel(nu, monkeypatch):
    from vargp_amd import noise
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.vargp_retrain import VARGPRetrain
    monkeypatch.setattr(orc, 'rbf_gram', lambda theta, x, y=None, full_gram=False: matern_ref(theta, x, y, nu=nu))
    S, F_, C, M, D, B = 2, 3, 3, 12, 6, 32
    params, prev, x, y, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=0, seed=3, kind='gauss')
    gp = _build(params, [], S, nu, MulticlassSoftmax(n_f=F_), cls=VARGPRetrain)
    with noise.inject(**to_dev(nz, DEV)):
        got = gp.loss(x.to(DEV), y.to(DEV))
    sum(got).backward()
    want64 = orc.loss(_dbl(params), [], _dbl(x), y, _dbl(nz))
    want32 = _one_thread(lambda: orc.loss(params, [], x, y, nz))
    floor = max(abs(a.item() - b.item()) / abs(b.item()) for a, b in zip(want32, want64) if b.item() != 0.0)
    for v, w in zip(got, want64):
        assert abs(v.item() - w.item()) <= (RTOL_SCALAR + 2.0 * floor) * abs(w.item())
