"""The natural-gradient q(u) fit on the device: ops.site_moments (csrc/sites.hip), VARGP.fit_q_newton_ (vargp_amd/sites.py) and the
factories' q_init='newton', against the fp64 restatement of tests/test_sites_host.py.

Rule: the tolerance is not fixed in advance.  For each checked quantity the error of the COMPOSED route (sites.composed_site_moments:
the per-op fp32 kernels) against the fp64 restatement is measured on the same inputs, and the fused kernel may be at most 4 x that
(the factor covers the different summation order over n and, in the MFMA, over Mt), with an absolute floor of one fp32 ulp of the
largest entry of the quantity.  Errors are max-abs.

Composed-route errors against fp64 (max-abs over the three outputs), as test_site_moments_against_fp64 printed them on an MI355X:
#  case (Mt, N, D, nu2, kind, shared y, w)            lam2      c         sum w ell  sum lam2
#  (1, 1, 1, 0, probit, per-output, None)             7.3e-08   3.6e-08   5.4e-08    7.3e-08
#  (63, 63, 32, 1, logit, shared, None)               4.6e-08   4.2e-07   8.5e-07    4.2e-07
#  (64, 65, 33, 3, poisson, per-output, zeros)        1.4e-07   9.9e-07   3.0e-06    1.5e-06
#  (65, 513, 40, 5, studentt, per-output, None)       1.0e-07   2.5e-06   2.8e-05    1.1e-05
#  (130, 513, 32, 0, studentt, shared, rand)          1.4e-07   1.3e-06   3.0e-05    1.3e-05
#  (130, 65, 40, 0, probit, per-output, None)         1.7e-07   6.2e-07   1.1e-06    3.0e-06
#  (65, 63, 1, 5, poisson, shared, None)              1.2e-07   8.2e-06   3.2e-06    3.1e-06
#  (64, 513, 33, 1, logit, per-output, rand)          8.6e-08   1.8e-06   1.3e-05    7.8e-06
# fit_q_newton_ (M = 20, D = 2, N = 300, C = 2), composed route against the restatement's converged q:
#  probit first task: u_mean 9.4e-06, L_u L_u^T 4.0e-07, bound 1.1e-05;  with a previous task: 2.1e-05, 2.0e-06, 2.0e-05
#  poisson first task: u_mean 5.1e-04, L_u L_u^T 6.9e-05, bound 1.9e-04;  with a previous task: 5.1e-04, 1.9e-04, 8.0e-04
"""
import math

import pytest
import torch

from test_collapsed import _Data, ref_vec2tril, ref_whiten
from test_sites_host import ref_newton, ref_sites

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP32 = float(torch.finfo(torch.float32).eps)
G = 3

# kind -> (restatement kind, ops kind, link code)
KIND = {'probit': ('bernoulli', (0,)), 'logit': ('bernoulli', (1,)), 'poisson': ('poisson', ()), 'studentt': ('studentt', None)}
DF = 4.0

# (Mt, N, D, nu2, kind, shared targets, weights): Mt on both sides of one and two 64-row panels, N around the 64-column step and
# over two chunks (513 > kMoMinChunk = 256), D on both sides of kRbfDirectD = 32, every kind with both distance forms;
# weights None | 'rand' | 'zeros' (random with exact zeros)
SITE_CASES = [
    (1, 1, 1, 0, 'probit', False, None),
    (63, 63, 32, 1, 'logit', True, None),
    (64, 65, 33, 3, 'poisson', False, 'zeros'),
    (65, 513, 40, 5, 'studentt', False, None),
    (130, 513, 32, 0, 'studentt', True, 'rand'),
    (130, 65, 40, 0, 'probit', False, None),
    (65, 63, 1, 5, 'poisson', True, None),
    (64, 513, 33, 1, 'logit', False, 'rand'),
    (200, 65, 33, 3, 'probit', True, 'rand'),       # four row panels, the last with 8 live rows; D % 32 == 1; a one-column tail
]


def _extra(kind, log_scale):
    from vargp_amd import ops
    okind, extra = KIND[kind]
    if kind == 'studentt':
        extra = (log_scale.to(DEV), DF, ops.studentt_lognorm(DF))
    return okind, extra


def _site_problem(Mt, N, D, kind, shared, wmode, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, generator=g)
    Z = torch.randn(G, Mt, D, generator=g)
    theta = torch.cat([math.log(0.8 * math.sqrt(D)) + 0.1 * torch.randn(D, generator=g), torch.tensor([math.log(0.9)])])
    alpha = 0.3 * torch.randn(G, Mt, generator=g) / math.sqrt(Mt)
    R = torch.randn(G, Mt, Mt, generator=g)
    Q = (10.0 / Mt ** 2) * (R @ R.mT)
    Q = 0.5 * (Q + Q.mT)
    shape = (N,) if shared else (G, N)
    if kind in ('probit', 'logit'):
        y = (torch.rand(shape, generator=g) < 0.5).float()
    elif kind == 'poisson':
        y = torch.poisson(1.5 * torch.ones(shape), generator=g)
    else:
        y = 0.3 * torch.randn(shape, generator=g)                 # |y - mu| well inside sqrt(df) sigma: no clamped point
    w = None if wmode is None else torch.rand(G, N, generator=g) + 0.25
    if wmode == 'zeros':
        w[:, torch.randperm(N, generator=g)[:N // 3]] = 0.0
    log_scale = torch.linspace(-0.2, 0.2, G)
    return dict(theta=theta, Z=Z, X=X, alpha=alpha, Q=Q, y=y, w=w, log_scale=log_scale, par=dict(log_scale=log_scale, df=DF))


def _dev(t):
    return None if t is None else t.to(DEV)


def _run(fn, pr, kind, nu2, X=None, y=None):
    okind, extra = _extra(kind, pr['log_scale'])
    out = fn(_dev(pr['theta']), _dev(pr['Z']), _dev(pr['X'] if X is None else X), _dev(pr['alpha']), _dev(pr['Q']),
             _dev(pr['y'] if y is None else y), _dev(pr['w']), okind, extra, nu2)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _hold(name, tag, fused, comp, ref):
    """fused error <= max(4 x composed error, one fp32 ulp of the largest entry)"""
    ef, ec = (fused.double() - ref).abs().max().item(), (comp.double() - ref).abs().max().item()
    floor = ULP32 * ref.abs().max().item()
    print(f'{tag} {name}: fused {ef:.3e} composed {ec:.3e} floor {floor:.3e}')
    assert ef <= max(4.0 * ec, floor), (tag, name, ef, ec, floor)


def _check_against_fp64(pr, kind, nu2, tag):
    from vargp_amd import ops, sites
    ref = ref_sites(kind, pr['par'], pr['theta'], pr['Z'], pr['X'], pr['alpha'], pr['Q'], pr['y'], pr['w'], nu2)
    comp = _run(sites.composed_site_moments, pr, kind, nu2)
    fused = _run(ops.site_moments, pr, kind, nu2)
    assert all(bool(torch.isfinite(t).all()) for t in fused)
    _hold('lam2', tag, fused[0], comp[0], ref['lam2'])
    _hold('c', tag, fused[1], comp[1], ref['c'])
    for j, name in ((0, 'sum_w_ell'), (1, 'sum_lam2'), (3, 'sum_w')):
        _hold(name, tag, fused[2][:, j], comp[2][:, j], ref['sums'][:, j])
    print(f'{tag} clamped: fused {fused[2][:, 2].tolist()} composed {comp[2][:, 2].tolist()} fp64 {ref["sums"][:, 2].tolist()}')
    assert torch.equal(fused[2][:, 2].double(), ref['sums'][:, 2])
    return ref, comp, fused


@pytest.mark.parametrize('case', SITE_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_site_moments_against_fp64(case):
    from vargp_amd import ops
    Mt, N, D, nu2, kind, shared, wmode = case
    pr = _site_problem(Mt, N, D, kind, shared, wmode, seed=100 + Mt + N + D)
    if N == 513:
        assert ops.site_moments_chunks(G, Mt, N, D) >= 2
    ref, _, fused = _check_against_fp64(pr, kind, nu2, str(case))
    if kind in ('probit', 'logit', 'poisson'):
        assert ref['sums'][:, 2].abs().max().item() == 0.0                          # log-concave: nothing to clamp
    if wmode == 'zeros':
        assert bool((fused[0][pr['w'] == 0] == 0).all())


@pytest.mark.parametrize('kind,D', [('poisson', 33), ('studentt', 2)])
def test_zero_weight_points_add_exactly_nothing(kind, D):
    """The rows of X and the targets of the zero-weight points replaced by NaN-free garbage: every output is bitwise unchanged."""
    from vargp_amd import ops
    N = 300
    pr = _site_problem(65, N, D, kind, False, 'zeros', seed=7)
    off = (pr['w'] == 0).all(0)
    assert 0 < int(off.sum()) < N
    g = torch.Generator().manual_seed(8)
    X2, y2 = pr['X'].clone(), pr['y'].clone()
    X2[off] = 37.5 * torch.randn(int(off.sum()), D, generator=g)
    y2[:, off] = 1e4
    a = _run(ops.site_moments, pr, kind, 0)
    b = _run(ops.site_moments, pr, kind, 0, X=X2, y=y2)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert bool((a[0][:, off] == 0).all())


def test_two_calls_are_bitwise_equal():
    from vargp_amd import ops
    pr = _site_problem(130, 513, 40, 'logit', False, 'rand', seed=9)
    a, b = _run(ops.site_moments, pr, 'logit', 3), _run(ops.site_moments, pr, 'logit', 3)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize('kind', ['probit', 'studentt'])
def test_variance_clamped_to_zero_at_an_inducing_point(kind):
    """x_5 = z_{0,2} and Q_0 with 2 / gamma^2 added at (2, 2): k^T Q k >= 2 gamma^2 there, var clamps to 0, and the quadrature's
    variance derivative -- and so lam2 -- is 0 by definition."""
    pr = _site_problem(5, 65, 2, kind, False, None, seed=11)
    pr['Q'] *= 0.1                                                # (at Mt = 5 the random Q alone would clamp most points)
    pr['X'][5] = pr['Z'][0, 2]
    pr['Q'][0, 2, 2] += 2.0 / math.exp(2.0 * pr['theta'][-1].item())
    ref, _, fused = _check_against_fp64(pr, kind, 0, f'clamp-var {kind}')
    assert ref['var'][0, 5].item() == 0.0 and ref['lam2'][0, 5].item() == 0.0 and fused[0][0, 5].item() == 0.0
    assert ref['var'][1, 5].item() > 0.0


def test_studentt_outlier_triggers_the_lam2_clamp():
    pr = _site_problem(63, 65, 33, 'studentt', False, None, seed=12)
    pr['y'][1, 7] += 50.0
    ref, _, fused = _check_against_fp64(pr, 'studentt', 5, 'outlier')
    assert ref['sums'][1, 2].item() >= 1.0 and ref['lam2'][1, 7].item() == 0.0 and fused[0][1, 7].item() == 0.0
    assert fused[2][:, 2].tolist() == ref['sums'][:, 2].tolist()


# -- fit_q_newton_ -------------------------------------------------------------------------------------------------------------------
def _model(kind, C, M, D, N, seed, prev=None):
    """A map_est model on synthetic data.  -> (gp on DEV, x, y float (C, N)), all built from `seed`."""
    from vargp_amd.kernels import RBFKernel
    from vargp_amd.likelihoods import BernoulliLikelihood, PoissonLikelihood
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, D, generator=g)
    f = torch.stack([torch.sin(1.5 * x[:, 0] + c) + 0.3 * x[:, -1] for c in range(C)])
    if kind == 'poisson':
        y, lik = torch.poisson((0.8 * f + 0.5).exp(), generator=g), PoissonLikelihood()
    else:
        y, lik = (torch.rand(C, N, generator=g) < torch.sigmoid(3.0 * f)).float(), BernoulliLikelihood(link=kind)
    z = torch.stack([x[torch.randperm(N, generator=g)[:M]] for _ in range(C)])
    torch.manual_seed(seed)
    kern = RBFKernel(D, map_est=True)
    gp = VARGP(z, kern, lik, n_var_samples=1, prev_params=prev).to(DEV)
    return gp, x, y


def _loss(gp, x, y):
    with torch.no_grad():
        _, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
        return float(kl_u) + float(nll)


def _state(gp):
    return gp.u_mean.detach().cpu().clone(), gp.u_tril_vec.detach().cpu().clone()


def _restate(gp, kind, x, y, state0, prev, start):
    M, C = gp.M, gp.z.shape[0]
    theta = gp.kernel.log_mean.detach().cpu()
    z_all = torch.cat([p['z'].cpu() for p in prev] + [gp.z.detach().cpu()], -2)
    rprev = [dict(u_mean=p['u_mean'].cpu(), u_tril=ref_vec2tril(p['u_tril_vec'].cpu(), p['z'].shape[-2])) for p in prev]
    u_mean0, u_tril0 = state0[0], ref_vec2tril(state0[1], M)
    if start == 'prior':                                          # q(u_t) = p(u_t | u_<): a_t = 0 and H_t = T_tt L_tt = I
        u_mean0, u_tril0 = torch.zeros(C, M, 1), ref_whiten(theta, z_all, rprev, 0)[0][:, -M:, -M:]
    return ref_newton(kind, {}, theta, z_all, rprev, x, y, None, 0, u_mean0, u_tril0)


def _fit_and_check(kind, C, M, D, N, seed, prev=None, expect_route='fused'):
    """Both routes from the same start against the restatement: the 4 x rule on u_mean, L_u L_u^T and the final bound; a rising
    trace; a higher bound and a lower kl_u + nll than at the start."""
    prev = prev or []
    start = 'prior' if kind == 'poisson' else 'current'           # (the default q(u) is too wide for Poisson: sites.fit_q_newton_)
    gp, x, y = _model(kind, C, M, D, N, seed, prev=[dict(p) for p in prev])
    state0 = _state(gp)
    before = _loss(gp, x, y)
    ref = _restate(gp, kind, x, y, state0, prev, start)
    assert ref['n_rejected'] == 0 and ref['n_iters'] < 20
    out = {}
    for route in ('composed', expect_route):
        with torch.no_grad():
            gp.u_mean.copy_(state0[0].to(DEV))
            gp.u_tril_vec.copy_(state0[1].to(DEV))
        fit = gp.fit_q_newton_(x.to(DEV), y.to(DEV), route=None if route == expect_route else route, start=start)
        assert fit.route == route
        Lu = ref_vec2tril(gp.u_tril_vec.detach().cpu(), M).double()
        out[route] = dict(fit=fit, u_mean=gp.u_mean.detach().cpu().squeeze(-1).double(), S_u=Lu @ Lu.mT, bound=fit.bound[-1])
        tr = fit.bound
        print(f'{kind} {route}: iters {fit.n_iters} (fp64 {ref["n_iters"]}) rejected {fit.n_rejected} clamped {fit.n_clamped} '
              f'trace {tr.sum(-1).tolist()}')
        assert tr.dtype == torch.float64 and tuple(tr.shape) == (fit.n_iters + 1, C) and fit.n_iters >= 1
        assert bool((tr[1:] >= tr[:-1]).all()) and bool((tr[-1] > tr[0]).all())
        assert fit.n_clamped == 0
    after = _loss(gp, x, y)
    print(f'{kind}: kl_u + nll {before:.4f} -> {after:.4f}')
    assert after < before
    if expect_route != 'composed':
        f, c = out[expect_route], out['composed']
        _hold('u_mean', kind, f['u_mean'], c['u_mean'], ref['u_mean'])
        _hold('S_u', kind, f['S_u'], c['S_u'], ref['S_u'])
        _hold('bound', kind, f['bound'], c['bound'], ref['trace'][-1])
        n = min(len(f['fit'].bound), len(c['fit'].bound), len(ref['trace']))
        _hold('trace', kind, f['fit'].bound[:n], c['fit'].bound[:n], ref['trace'][:n])
    return gp, out, ref


@pytest.mark.parametrize('kind', ['probit', 'poisson'])
def test_fit_first_task(kind):
    _fit_and_check(kind, C=2, M=20, D=2, N=300, seed=22)


@pytest.mark.parametrize('kind', ['probit', 'poisson'])
def test_fit_with_one_previous_task(kind):
    gp0, _, _ = _fit_and_check(kind, C=2, M=20, D=2, N=300, seed=22)
    prev = [dict(z=gp0.z.detach().clone(), u_mean=gp0.u_mean.detach().clone(), u_tril_vec=gp0.u_tril_vec.detach().clone())]
    _fit_and_check(kind, C=2, M=20, D=2, N=300, seed=23, prev=prev)


def test_above_the_lds_limit_takes_the_composed_route():
    """Mt = 260 > ops.SITE_MAX_MT: the default route is the composed one; a rising trace, a higher bound, a lower loss, and the
    final bound of the restatement to 1e-3 (the fp32 factorisation of a 260 x 260 kernel matrix whose condition number reaches
    gamma^2 M / jitter ~ 1e6 carries the log-determinant of the KL term to about 1e-7 * 1e6 * 1e-2 relative)."""
    from vargp_amd import ops
    assert 260 > ops.SITE_MAX_MT
    gp, out, ref = _fit_and_check('probit', C=1, M=260, D=2, N=300, seed=24, expect_route='composed')
    got = out['composed']['bound']
    assert torch.allclose(got, ref['trace'][-1], rtol=1e-3, atol=0.0), (got, ref['trace'][-1])


@pytest.mark.parametrize('which', ['clf', 'reg'])
def test_factories_q_init_newton(which):
    """The same factory call with and without q_init='newton' (same seed: same inducing points and start): q(u) differs and the
    full-batch kl_u + nll is lower."""
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(31)
    x = torch.randn(200, 2, generator=g)
    f = torch.sin(1.5 * x[:, 0]) + 0.3 * x[:, 1]
    if which == 'clf':
        data = _Data(x, (f > 0).long())
        make = lambda **kw: VARGP.create_clf(data, M=10, likelihood='bernoulli', map_est_hypers=True, n_var_samples=1, **kw)
        y = data.targets
    else:
        data = _Data(x, torch.poisson((0.8 * f + 0.5).exp(), generator=g))
        make = lambda **kw: VARGP.create_reg(data, M=10, likelihood='poisson', map_est_hypers=True, n_var_samples=1, **kw)
        y = data.targets
    models = {}
    for q_init in ('default', 'newton'):
        torch.manual_seed(5)
        models[q_init] = make(q_init=q_init, newton_iters=20) if q_init == 'newton' else make()
        assert models[q_init].z.device.type == 'cpu'
    a, b = models['default'], models['newton']
    assert torch.equal(a.z, b.z) and not torch.equal(a.u_mean, b.u_mean) and not torch.equal(a.u_tril_vec, b.u_tril_vec)
    la, lb = _loss(a.to(DEV), x, y), _loss(b.to(DEV), x, y)
    print(f'{which}: kl_u + nll default {la:.4f} newton {lb:.4f}')
    assert lb < la
