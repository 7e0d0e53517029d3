"""The differentiable site bound on the device: ops.site_bound_diff / ops.site_bound_bwd (csrc/sites.hip: vargp_site_bound_bwd),
VARGP.site_bound, VARGP.fit_sites_ and the factories' q_init='em', against the fp64 restatement of tests/test_site_bound_host.py.

Rule (that of tests/test_hip_sites.py): no tolerance is fixed in advance.  For each gradient the max-abs error of the COMPOSED
route (sites.composed_site_bound: the per-op fp32 kernels, fp64 accumulation over tiles) against the fp64 restatement is measured
on the same input, and the fused kernel may be at most 4 x that, with a floor of one fp32 ulp of the quantity's largest entry.

Composed-route errors against fp64 (max-abs), as test_gradients_against_fp64 printed them on an MI355X:
#  case (Mt, N, D, nu2, kind, shared y, w)            gtheta    gZ        galpha    gQ        gls
#  (1, 1, 1, 0, probit, per-output, None)             2.2e-06   3.9e-07   4.5e-08   5.6e-09   -
#  (63, 63, 32, 1, logit, shared, None)               3.3e-06   3.4e-09   7.6e-07   1.5e-07   -
#  (64, 65, 33, 3, poisson, per-output, zeros)        3.1e-06   1.9e-08   1.2e-06   5.2e-07   -
#  (65, 513, 40, 5, studentt, per-output, None)       2.8e-05   1.3e-07   5.8e-06   1.2e-05   7.9e-06
#  (130, 513, 32, 0, studentt, shared, rand)          2.3e-04   7.7e-08   5.7e-06   2.0e-05   4.7e-06
#  (130, 65, 40, 0, probit, per-output, None)         1.3e-05   9.1e-09   9.9e-07   8.3e-07   -
#  (65, 63, 1, 5, poisson, shared, None)              3.1e-06   8.5e-07   2.5e-05   8.6e-08   -
#  (64, 513, 33, 1, logit, per-output, rand)          3.2e-06   1.6e-08   2.9e-06   1.8e-06   -
#  (256, 65, 33, 0, studentt, per-output, rand)       1.5e-05   7.4e-09   4.4e-07   8.4e-07   1.5e-06
# VARGP.site_bound (M = 20, D = 2, N = 300, C = 2), composed route against the restatement (z, log_mean, log_scale, bound):
#  probit first task: 5.2e-03, 8.8e-05, -, 2.2e-05;  with a previous task: 8.5e-04, 4.9e-04, -, 3.2e-05
#  studentt first task: 3.9e-03, 1.7e-03, 2.8e-04, 2.1e-04;  with a previous task: 3.0e-02, 3.6e-02, 2.2e-03, 1.3e-03
"""
import math

import pytest
import torch

from test_collapsed import _Data, ref_vec2tril
from test_hip_sites import DEV, DF, G, SITE_CASES, ULP32, _dev, _extra, _site_problem
from test_site_bound_host import ref_data_term, ref_site_bound

pytestmark = pytest.mark.gpu
CASES = SITE_CASES + [(256, 65, 33, 0, 'studentt', False, 'rand')]
SEED = torch.tensor([1.0, -0.5, 2.0])                                   # per-output seeds that are not all 1
NAMES = ('gtheta', 'gZ', 'galpha', 'gQ', 'gls')


def _hold(name, tag, fused, comp, ref):
    """fused error <= max(4 x composed error, one fp32 ulp of the largest entry)"""
    ef, ec = (fused.double() - ref).abs().max().item(), (comp.double() - ref).abs().max().item()
    floor = ULP32 * ref.abs().max().item()
    print(f'{tag} {name}: fused {ef:.3e} composed {ec:.3e} floor {floor:.3e}')
    assert ef <= max(4.0 * ec, floor), (tag, name, ef, ec, floor)


def _device_grads(fn, pr, kind, nu2, X=None, y=None):
    """value and the gradients of sum_g SEED_g value_g for (theta, Z, alpha, Q[, log_scale]) from an autograd node on the device."""
    okind, extra = _extra(kind, pr['log_scale'])
    leaves = [_dev(pr[k]).clone().requires_grad_(True) for k in ('theta', 'Z', 'alpha', 'Q')]
    if kind == 'studentt':
        leaves.append(extra[0].clone().requires_grad_(True))
        extra = (leaves[-1],) + tuple(extra[1:])
    val = fn(leaves[0], leaves[1], _dev(pr['X'] if X is None else X), leaves[2], leaves[3], _dev(pr['y'] if y is None else y),
             _dev(pr['w']), okind, extra, nu2)
    grads = torch.autograd.grad((val * SEED.to(DEV).to(val.dtype)).sum(), leaves)
    torch.cuda.synchronize()
    out = dict(zip(NAMES, [g.cpu() for g in grads]))
    out['value'] = val.detach().cpu()
    return out


def _ref_grads(pr, kind, nu2):
    leaves = [pr[k].double().clone().requires_grad_(True) for k in ('theta', 'Z', 'alpha', 'Q', 'log_scale')]
    par = dict(log_scale=leaves[4], df=DF)
    val = ref_data_term(kind, par, leaves[0], leaves[1], pr['X'], leaves[2], leaves[3], pr['y'], pr['w'], nu2)
    grads = torch.autograd.grad((val * SEED.double()).sum(), leaves, allow_unused=True)
    out = {k: g for k, g in zip(NAMES, grads) if g is not None}
    out['value'] = val.detach()
    return out


def _check(pr, kind, nu2, tag):
    from vargp_amd import ops, sites
    ref = _ref_grads(pr, kind, nu2)
    comp = _device_grads(sites.composed_site_bound, pr, kind, nu2)
    fused = _device_grads(ops.site_bound_diff, pr, kind, nu2)
    row = []
    for name in NAMES:
        if name in fused:
            assert bool(torch.isfinite(fused[name]).all()), name
            _hold(name, tag, fused[name], comp[name], ref[name])
            row.append(f'{(comp[name].double() - ref[name]).abs().max().item():.1e}')
    print(f'{tag} composed row (gtheta gZ galpha gQ gls): ' + '   '.join(row))
    assert torch.equal(fused['gQ'], fused['gQ'].mT)
    return ref, comp, fused


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_gradients_against_fp64(case):
    """gZ, gtheta (all D + 1 entries), galpha, gQ and gls of sum_g s_g value_g at SITE_CASES' shapes and at Mt = 256."""
    from vargp_amd import ops
    Mt, N, D, nu2, kind, shared, wmode = case
    pr = _site_problem(Mt, N, D, kind, shared, wmode, seed=100 + Mt + N + D)
    if N == 513:
        assert ops.site_bound_bwd_chunks(G, Mt, N, D) >= 2
    _check(pr, kind, nu2, str(case))


@pytest.mark.parametrize('case', [CASES[3], CASES[2]], ids=lambda c: '-'.join(str(v) for v in c))
def test_forward_value_is_bitwise_site_moments(case):
    from vargp_amd import ops
    Mt, N, D, nu2, kind, shared, wmode = case
    pr = _site_problem(Mt, N, D, kind, shared, wmode, seed=3)
    okind, extra = _extra(kind, pr['log_scale'])
    args = (_dev(pr['theta']), _dev(pr['Z']), _dev(pr['X']), _dev(pr['alpha']), _dev(pr['Q']), _dev(pr['y']), _dev(pr['w']), okind,
            extra, nu2)
    assert torch.equal(ops.site_bound_diff(*args), ops.site_moments(*args)[2][:, 0])


def _bwd(pr, kind, nu2, X=None, y=None):
    from vargp_amd import ops
    okind, extra = _extra(kind, pr['log_scale'])
    out = ops.site_bound_bwd(_dev(pr['theta']), _dev(pr['Z']), _dev(pr['X'] if X is None else X), _dev(pr['alpha']), _dev(pr['Q']),
                             _dev(pr['y'] if y is None else y), _dev(pr['w']), okind, extra, SEED.to(DEV), nu2)
    gQ = -ops.gram_moments(_dev(pr['theta']), _dev(pr['Z']), _dev(pr['X'] if X is None else X), out[3], out[3], nu2)[0]
    torch.cuda.synchronize()
    return [t.cpu() for t in out if t is not None] + [gQ.cpu()]


@pytest.mark.parametrize('kind,D', [('poisson', 33), ('studentt', 2)])
def test_zero_weight_points_add_exactly_nothing(kind, D):
    """The rows of X of the zero-weight points overwritten with 1e30 and their targets with NaN: every output of the backward
    (gZ, gtheta, galpha, gv, gls) and gQ is bitwise unchanged, and gv is 0 there."""
    N = 300
    pr = _site_problem(65, N, D, kind, False, 'zeros', seed=7)
    off = (pr['w'] == 0).all(0)
    assert 0 < int(off.sum()) < N
    X2, y2 = pr['X'].clone(), pr['y'].clone()
    X2[off] = 1e30
    y2[:, off] = float('nan')
    a, b = _bwd(pr, kind, 0), _bwd(pr, kind, 0, X=X2, y=y2)
    for u, v in zip(a, b):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v)
    assert bool((a[3][:, off] == 0).all())


def test_two_calls_are_bitwise_equal():
    pr = _site_problem(130, 513, 40, 'logit', False, 'rand', seed=9)
    for u, v in zip(_bwd(pr, 'logit', 3), _bwd(pr, 'logit', 3)):
        assert torch.equal(u, v)


@pytest.mark.parametrize('kind', ['probit', 'studentt'])
def test_variance_clamp_passes_no_gradient(kind):
    """x_5 = z_{0,2} and Q_0 with 2 / gamma^2 added at (2, 2): gamma^2 - k^T Q k < 0 there, gv is exactly 0 and the gradients are
    the restatement's, whose autograd gives 0 through clamp_min."""
    pr = _site_problem(5, 65, 2, kind, False, None, seed=11)
    pr['Q'] *= 0.1                                                # (at Mt = 5 the random Q alone would clamp most points)
    pr['X'][5] = pr['Z'][0, 2]
    pr['Q'][0, 2, 2] += 2.0 / math.exp(2.0 * pr['theta'][-1].item())
    _check(pr, kind, 0, f'clamp-var {kind}')
    gv = _bwd(pr, kind, 0)[3]
    assert gv[0, 5].item() == 0.0 and gv[1, 5].item() != 0.0


def test_studentt_outlier_keeps_the_sign_of_dvar():
    """test_hip_sites' outlier: d ell / d var > 0 at (1, 7), where lam2 is clamped to 0.  gv keeps the true sign (SEED_1 < 0, so
    gv < 0 there while every regular point of output 1 has gv > 0) and gQ matches fp64 -- it would not if lam2 were reused."""
    from test_sites_host import ref_sites
    pr = _site_problem(63, 65, 33, 'studentt', False, None, seed=12)
    pr['y'][1, 7] += 50.0
    ref = ref_sites('studentt', pr['par'], pr['theta'], pr['Z'], pr['X'], pr['alpha'], pr['Q'], pr['y'], pr['w'], 5)
    assert ref['lam2'][1, 7].item() == 0.0 and ref['sums'][1, 2].item() >= 1.0
    _, _, fused = _check(pr, 'studentt', 5, 'outlier')
    gv = _bwd(pr, 'studentt', 5)[3]
    assert gv[1, 7].item() * SEED[1].item() > 0.0
    assert int((gv[1] * SEED[1] > 0).sum()) == int(ref['sums'][1, 2].item())


# -- VARGP.site_bound ----------------------------------------------------------------------------------------------------------------
def _model(kind, C, M, D, N, seed, prev=None, nu=None, lengthscale=None):
    """A map_est model on synthetic data (test_hip_sites._model, with Student-t and a Matern option).  -> gp on DEV, x, y (C, N)."""
    from vargp_amd.kernels import MaternKernel, RBFKernel
    from vargp_amd.likelihoods import BernoulliLikelihood, PoissonLikelihood, StudentTLikelihood
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, D, generator=g)
    f = torch.stack([torch.sin(1.5 * x[:, 0] + c) + 0.3 * x[:, -1] for c in range(C)])
    if kind == 'poisson':
        y, lik = torch.poisson((0.8 * f + 0.5).exp(), generator=g), PoissonLikelihood()
    elif kind == 'studentt':
        y, lik = f + 0.2 * torch.randn(C, N, generator=g), StudentTLikelihood(C, df=DF, init_log_scale=-1.0)
    else:
        y, lik = (torch.rand(C, N, generator=g) < torch.sigmoid(3.0 * f)).float(), BernoulliLikelihood(link=kind)
    z = torch.stack([x[torch.randperm(N, generator=g)[:M]] for _ in range(C)])
    torch.manual_seed(seed)
    kern = RBFKernel(D, map_est=True) if nu is None else MaternKernel(D, nu=nu, map_est=True)
    if lengthscale is not None:
        with torch.no_grad():
            kern.log_mean[:D] = math.log(lengthscale)
    return VARGP(z, kern, lik, n_var_samples=1, prev_params=prev).to(DEV), x, y


def _model_grads(gp, x, y, route):
    bound = gp.site_bound(x.to(DEV), y.to(DEV), route=route)
    params = [gp.z, gp.kernel.log_mean] + ([gp.likelihood.log_scale] if gp.likelihood.kind == 'studentt' else [])
    grads = torch.autograd.grad(bound.sum(), params)
    torch.cuda.synchronize()
    return bound.detach().cpu(), [g.cpu() for g in grads]


@pytest.mark.parametrize('with_prev', [False, True], ids=['first', 'prev'])
@pytest.mark.parametrize('kind', ['probit', 'studentt'])
def test_model_site_bound(kind, with_prev):
    """M = 20, D = 2, N = 300, C = 2: the value is fit_q_newton_(n_iters=0).bound[0] bit for bit (the same forward pass at the same
    alpha, Q and the same KL term: both come from whitened.py, the fit's under no_grad, the bound's on the graph), and
    torch.autograd.grad for z, log_mean and log_scale holds the 4 x rule against the restatement on both routes' shapes ('composed'
    forced at the same shape)."""
    from vargp_amd import sites
    C, M, D, N = 2, 20, 2, 300
    prev = []
    if with_prev:
        gp0, x0, y0 = _model(kind, C, M, D, N, seed=22)
        gp0.fit_q_newton_(x0.to(DEV), y0.to(DEV), n_iters=3)
        prev = [dict(z=gp0.z.detach().clone(), u_mean=gp0.u_mean.detach().clone(), u_tril_vec=gp0.u_tril_vec.detach().clone())]
    gp, x, y = _model(kind, C, M, D, N, seed=23, prev=[dict(p) for p in prev])
    gp.fit_q_newton_(x.to(DEV), y.to(DEV), n_iters=2)              # a q(u) away from the default start
    fit0 = gp.fit_q_newton_(x.to(DEV), y.to(DEV), n_iters=0)
    fused_val, fused = _model_grads(gp, x, y, None)
    comp_val, comp = _model_grads(gp, x, y, 'composed')
    print(f'{kind} prev={with_prev}: bound {fused_val.tolist()} fit_q_newton_(0) {fit0.bound[0].tolist()}')
    assert torch.equal(fused_val, fit0.bound[0])
    # the restatement at the model's parameters and its whitened q
    a_t, H_t = (t.cpu().double() for t in sites.whitened_q(gp))
    rprev = [dict(u_mean=p['u_mean'].cpu().double(), u_tril=ref_vec2tril(p['u_tril_vec'].cpu(), M).double()) for p in prev]
    z_lt = torch.cat([p['z'].cpu() for p in prev], -2).double() if prev else torch.zeros(C, 0, D, dtype=torch.float64)
    leaves = [gp.z.detach().cpu().double().requires_grad_(True), gp.kernel.log_mean.detach().cpu().double().requires_grad_(True)]
    par = {}
    if kind == 'studentt':
        leaves.append(gp.likelihood.log_scale.detach().cpu().double().requires_grad_(True))
        par = dict(log_scale=leaves[2], df=DF)
    val = ref_site_bound(kind, par, leaves[1], z_lt, leaves[0], rprev, x, y, None, 0, a_t, H_t)
    ref = torch.autograd.grad(val.sum(), leaves)
    for name, f, c, r in zip(('z', 'log_mean', 'log_scale'), fused, comp, ref):
        _hold(name, f'{kind} prev={with_prev}', f, c, r)
    _hold('bound', f'{kind} prev={with_prev}', fused_val, comp_val, val.detach())


def test_above_the_lds_limit_takes_the_composed_route():
    """Mt = 260 over two tasks: the default route is the composed one, and its gradients are finite."""
    from vargp_amd import ops, sites
    assert sites.pick_route(None, 260, 'site_bound') == 'composed' and 260 > ops.SITE_MAX_MT
    gp0, _, _ = _model('probit', 1, 130, 2, 300, seed=24)
    prev = [dict(z=gp0.z.detach().clone(), u_mean=0.1 * gp0.u_mean.detach().clone(), u_tril_vec=gp0.u_tril_vec.detach().clone())]
    gp, x, y = _model('probit', 1, 130, 2, 300, seed=25, prev=prev)
    with pytest.raises(ValueError, match='256'):
        gp.site_bound(x.to(DEV), y.to(DEV), route='fused')
    val, grads = _model_grads(gp, x, y, None)
    assert bool(torch.isfinite(val).all()) and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)


# -- fit_sites_ ----------------------------------------------------------------------------------------------------------------------
def _toy(kind, seed=0):
    """The toy start of tests/test_collapsed_grad.py for counts and labels: x ~ U(-2.5, 2.5), a latent sin(3 x) that needs a
    lengthscale near 0.5, a Matern-1/2 model started ten times too long, M = 10 inducing points at random data points."""
    from test_collapsed_grad import TOY_LENGTHSCALE, TOY_START
    from vargp_amd.kernels import MaternKernel
    from vargp_amd.likelihoods import BernoulliLikelihood, PoissonLikelihood
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(seed)
    x = 5.0 * torch.rand(400, 1, generator=g) - 2.5
    f = torch.sin(3.0 * x[:, 0])
    if kind == 'poisson':
        y, lik = torch.poisson((1.2 * f + 0.5).exp(), generator=g).unsqueeze(0), PoissonLikelihood()
    else:
        y, lik = (torch.rand(400, generator=g) < torch.sigmoid(4.0 * f)).float().unsqueeze(0), BernoulliLikelihood(link='probit')
    z = x[torch.randperm(400, generator=g)[:10]].unsqueeze(0)
    torch.manual_seed(seed)
    kern = MaternKernel(1, nu=0.5, map_est=True)
    with torch.no_grad():
        kern.log_mean[0] = math.log(TOY_START * TOY_LENGTHSCALE)
    return VARGP(z, kern, lik, n_var_samples=1).to(DEV), x.to(DEV), y.to(DEV)


@pytest.mark.parametrize('kind', ['probit', 'poisson'])
def test_fit_sites_on_the_toy_start(kind):
    """start='prior': every row-sum of the trace is non-decreasing, the final bound exceeds fit_q_newton_'s alone on the same start
    (the lengthscale is ten times too long there), and u_mean / u_tril_vec are whitened_q's q at the final parameters: writing
    whitened_q back with set_whitened_q_ changes them by less than 1e-3 of their largest entry (the fp32 round trip through
    T_tt and L_tt, whose condition number is at most (gamma^2 M / jitter)^1/2 ~ 3e2, costs about 3e2 x 1e-7 per product)."""
    from vargp_amd import sites
    gp, x, y = _toy(kind)
    alone = gp.fit_q_newton_(x, y, start='prior').bound[-1].sum().item()
    gp, x, y = _toy(kind)
    fit = gp.fit_sites_(x, y, n_rounds=3, m_steps=15, lr=5e-2, start='prior')
    sums = fit.bound.sum(-1)
    print(f'{kind}: fit_q_newton_ alone {alone:.3f}; EM trace {sums.tolist()} rounds {fit.n_rounds} newton {fit.n_newton} '
          f'stopped {fit.stopped}; lengthscale {gp.kernel.log_mean[0].exp().item():.3f}')
    assert fit.bound.dtype == torch.float64 and tuple(fit.bound.shape) == (fit.n_rounds + 1, 1) and fit.n_rounds >= 1
    assert bool((sums[1:] >= sums[:-1]).all()) and bool(torch.isfinite(sums).all())
    assert sums[-1].item() > alone
    before = gp.u_mean.detach().clone(), gp.u_tril_vec.detach().clone()
    sites.set_whitened_q_(gp, *sites.whitened_q(gp))
    for u, v in zip(before, (gp.u_mean.detach(), gp.u_tril_vec.detach())):
        assert (u - v).abs().max().item() <= 1e-3 * u.abs().max().item()


@pytest.mark.parametrize('which', ['clf', 'poisson', 'studentt'])
def test_factories_q_init_em(which):
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(31)
    x = torch.randn(200, 2, generator=g)
    f = torch.sin(1.5 * x[:, 0]) + 0.3 * x[:, 1]
    kw = dict(M=10, map_est_hypers=True, n_var_samples=1, q_init='em', em_rounds=2, em_steps=5)
    torch.manual_seed(5)
    if which == 'clf':
        data = _Data(x, (f > 0).long())
        gp = VARGP.create_clf(data, likelihood='bernoulli', **kw)
    elif which == 'poisson':
        data = _Data(x, torch.poisson((0.8 * f + 0.5).exp(), generator=g))
        gp = VARGP.create_reg(data, likelihood='poisson', **kw)
    else:
        data = _Data(x, f + 0.1 * torch.randn(200, generator=g))
        gp = VARGP.create_reg(data, likelihood='studentt', **kw)
    assert gp.z.device.type == 'cpu'
    gp = gp.to(DEV)
    with torch.no_grad():
        parts = gp.loss(x.to(DEV), data.targets.to(DEV))
    assert all(math.isfinite(float(p)) for p in parts)
