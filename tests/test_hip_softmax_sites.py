"""The natural-gradient q(u) fit for MulticlassSoftmax on the device: ops.site_marginals (csrc/sites.hip), ops.softmax_sites and
ops.softmax_site_noise (csrc/softmax_sites.hip), ops.gram_moments_v (csrc/moments.hip), VARGP.fit_q_softmax_ (vargp_amd/sites.py)
and create_clf(q_init='newton_softmax'), against the fp64 restatement of tests/test_softmax_sites_host.py.

Rule, as in tests/test_hip_sites.py: the tolerance is not fixed in advance.  For each checked quantity the error of the COMPOSED
route (sites.composed_softmax_marginals: gram op + ops.bgemm; sites.composed_softmax_sites: fp32 elementwise torch; ops.gram_moments
for gram_moments_v) against the fp64 restatement is measured on the same inputs, and the new kernel may be at most 4 x that, with an
absolute floor of one fp32 ulp of the largest entry of the quantity.  Errors are max-abs.

Composed-route errors against fp64 (max-abs), as the tests printed them on an MI355X:
#  site_marginals (Mt, N, D, nu2)   mu        var           softmax_sites (C, N, F, w)   lam1      lam2      sum w ell  sum lam2
#  (1, 1, 1, 0)                     1.0e-08   5.2e-08       (2, 1, 1, None)              1.3e-07   2.8e-08   1.7e-07    2.9e-08
#  (63, 63, 32, 1)                  1.5e-08   6.3e-08       (3, 63, 4, rand)             1.9e-07   4.5e-08   2.4e-06    9.0e-07
#  (64, 65, 33, 3), Q x 4           3.6e-08   1.4e-07       (10, 65, 10, zeros), +-60    5.6e-30   1.6e-30   1.0e-04    8.2e-31
#  (130, 513, 40, 5)                4.9e-08   8.1e-08       (16, 65, 2, None)            2.1e-07   4.5e-08   9.7e-06    9.8e-07
#  (200, 65, 33, 0)                 5.4e-08   8.2e-08       (17, 513, 3, rand)           6.3e-07   8.2e-08   9.3e-05    1.8e-05
#  (256, 130, 2, 0)                 9.7e-08   1.6e-07       (33, 300, 2, zeros)          2.8e-07   4.3e-08   3.0e-05    1.5e-07
#                                                           (128, 70, 2, None)           1.8e-07   3.2e-08   7.4e-06    5.0e-08
# gram_moments' own error of c: (130, 1000, 40, 1, 0, rand) 2.7e-06, (33, 64, 32, 1, 3, zeros) 3.5e-07
# fit_q_softmax_ (4 iterations), composed route against the restatement: u_mean, L_u L_u^T, trace
#  first task 1.0e-06, 1.5e-07, 5.7e-06;  with a previous task 4.0e-06, 5.3e-07, 1.5e-04;  Matern 3/2 6.5e-07, 8.5e-08, 9.2e-06
# smallest decision margin of the restatement: first 7.6e-03, previous task 3.4e-03, Matern 4.5e-03, Mt = 260 4.5e-03

The fit tests take the device's own noise (ops.softmax_site_noise) to the restatement and assert that every accept / reject
decision of the restatement within the 4 iterations has a relative margin of at least 1e-3 of |bound|; the data seeds below were
chosen so that the restatement alone, on a numpy restatement of the same Philox stream, satisfies it (FIT_SEEDS)."""
import math

import numpy as np
import pytest
import torch

from test_collapsed import _Data, ref_kernel, ref_moments, ref_vec2tril, ref_whiten
from test_hip_collapsed import _moment_problem
from test_hip_rng import _normal_ref
from test_hip_sites import _hold, _site_problem
from test_softmax_sites_host import blobs, ref_softmax_newton, ref_softmax_sites

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F64 = torch.float64
G = 3
NOISE_STREAM = 2                 # kStreamSite (csrc/softmax_sites.hip)


def _dev(t):
    return None if t is None else t.to(DEV)


# -- site_marginals -----------------------------------------------------------------------------------------------------------------
# (Mt, N, D, nu2): both sides of one, two and four row panels, the 64-column step, two chunks (513 > 256), both distance forms
# (D <= 32 | > 32), every epilogue
MARGINAL_CASES = [(1, 1, 1, 0), (63, 63, 32, 1), (64, 65, 33, 3), (130, 513, 40, 5), (200, 65, 33, 0), (256, 130, 2, 0)]
CLAMP_CASE, CLAMP_Q_SCALE = (64, 65, 33, 3), 4.0                  # Q scaled up until some, not all, variances clamp to exactly 0


@pytest.mark.parametrize('case', MARGINAL_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_site_marginals_against_fp64(case):
    from vargp_amd import ops, sites
    Mt, N, D, nu2 = case
    pr = _site_problem(Mt, N, D, 'probit', True, None, seed=300 + Mt + N + D)
    if case == CLAMP_CASE:
        pr['Q'] = pr['Q'] * CLAMP_Q_SCALE
    if N == 513:
        assert ops.site_moments_chunks(G, Mt, N, D) >= 2
    th, Z, X, al, Q = (pr[k].to(F64) for k in ('theta', 'Z', 'X', 'alpha', 'Q'))
    K = ref_kernel(Z, X.unsqueeze(0), th, nu2)
    ref_mu = (al.unsqueeze(-1) * K).sum(-2)
    ref_var = ((2.0 * th[-1]).exp() - (K * (Q @ K)).sum(-2)).clamp_min(0.0)
    args = [_dev(pr[k]) for k in ('theta', 'Z', 'X', 'alpha', 'Q')]
    fused = [t.cpu() for t in ops.site_marginals(*args, nu2)]
    again = [t.cpu() for t in ops.site_marginals(*args, nu2)]
    comp = [t.cpu() for t in sites.composed_softmax_marginals(*args, nu2)]
    assert all(tuple(t.shape) == (G, N) and bool(torch.isfinite(t).all()) for t in fused)
    assert torch.equal(fused[0], again[0]) and torch.equal(fused[1], again[1])
    assert bool((fused[1] >= 0).all())
    _hold('mu', str(case), fused[0], comp[0], ref_mu)
    _hold('var', str(case), fused[1], comp[1], ref_var)
    if case == CLAMP_CASE:
        zero = ref_var == 0
        # where fp64 clamps with a margin of 1e-4 gamma^2 (far above the fp32 error of k^T Q k), the kernel's variance is exactly 0
        sure = ((2.0 * th[-1]).exp() - (K * (Q @ K)).sum(-2)) < -1e-4 * (2.0 * th[-1]).exp()
        print(f'{case}: {int(zero.sum())} of {zero.numel()} variances clamp in fp64, {int((fused[1] == 0).sum())} in the kernel')
        assert 0 < int(sure.sum()) and int(zero.sum()) < zero.numel() and bool((fused[1][sure] == 0).all())


# -- softmax_sites ------------------------------------------------------------------------------------------------------------------
# (C, N, F, weights): two classes and one point; both sides of the 64-point step; the register path (C <= 16) and the LDS path on
# both sides of 16, C not a multiple of 4, the limit C = 128; 513 points
SOFTMAX_CASES = [(2, 1, 1, None), (3, 63, 4, 'rand'), (10, 65, 10, 'zeros'), (16, 65, 2, None), (17, 513, 3, 'rand'),
                 (33, 300, 2, 'zeros'), (128, 70, 2, None)]
EXTREME_CASE = (10, 65, 10, 'zeros')                               # rows of mu at +-60


def _softmax_problem(C, N, F, wmode, seed):
    g = torch.Generator().manual_seed(seed)
    mu = 2.0 * torch.randn(C, N, generator=g)
    var = torch.rand(C, N, generator=g) * 2.0
    var[:, ::5] = 0.0
    var[0, :] = 0.0
    if (C, N, F, wmode) == EXTREME_CASE:
        mu[0], mu[1] = 60.0, -60.0
    y = torch.randint(0, C, (N,), generator=g)
    w = None if wmode is None else torch.rand(N, generator=g) + 0.25
    if wmode == 'zeros':
        w[torch.randperm(N, generator=g)[:N // 3]] = 0.0
    return mu, var, y, w


@pytest.mark.parametrize('case', SOFTMAX_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_softmax_sites_against_fp64(case):
    from vargp_amd import ops, sites
    C, N, F, wmode = case
    seed = 1000 + C + N
    mu, var, y, w = _softmax_problem(C, N, F, wmode, seed)
    eps = ops.softmax_site_noise(seed, F, C, N, device=DEV)
    assert tuple(eps.shape) == (F, C, N)
    ref = ref_softmax_sites(mu, var, y, w, eps.cpu())
    run = lambda fn, **kw: [t.cpu() for t in fn(_dev(mu), _dev(var), _dev(y), _dev(w), **kw)]
    fused = run(ops.softmax_sites, n_f=F, eps=eps)
    comp = run(sites.composed_softmax_sites, eps=eps)
    assert all(bool(torch.isfinite(t).all()) for t in fused) and bool((fused[1] >= 0).all())
    tag = str(case)
    _hold('lam1', tag, fused[0], comp[0], ref['lam1'])
    _hold('lam2', tag, fused[1], comp[1], ref['lam2'])
    for j, name in ((0, 'sum_w_ell'), (1, 'sum_lam2'), (3, 'sum_w')):
        _hold(name, tag, fused[2][j], comp[2][j], ref['sums'][j])
    assert fused[2][2].item() == ref['sums'][2].item()
    # the noise generated inside the kernel is the noise softmax_site_noise writes; two calls are bitwise equal
    own = run(ops.softmax_sites, n_f=F, seed=seed)
    again = run(ops.softmax_sites, n_f=F, seed=seed)
    for u, v, t in zip(fused, own, again):
        assert torch.equal(u, v) and torch.equal(v, t)
    if wmode == 'zeros':
        off = w == 0
        assert 0 < int(off.sum()) < N and bool((fused[0][:, off] == 0).all()) and bool((fused[1][:, off] == 0).all())
        # finite garbage in the zero-weight points' mu, var and y: every output is bitwise unchanged
        g = torch.Generator().manual_seed(5)
        mu2, var2, y2 = mu.clone(), var.clone(), y.clone()
        mu2[:, off] = 1e4 * torch.randn(C, int(off.sum()), generator=g)
        var2[:, off] = 1e6
        y2[off] = (y[off] + 1) % C
        other = [t.cpu() for t in ops.softmax_sites(_dev(mu2), _dev(var2), _dev(y2), _dev(w), F, seed=seed)]
        for u, v in zip(own, other):
            assert torch.equal(u, v)


def test_softmax_sites_refuses_more_than_128_classes():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    mu = torch.zeros(129, 4, device=DEV)
    with pytest.raises(VargpHipError, match='128'):
        ops.softmax_sites(mu, mu, torch.zeros(4, dtype=torch.int64, device=DEV), None, 2)
    with pytest.raises(VargpHipError, match='128'):
        ops.softmax_site_noise(0, 2, 129, 4, device=DEV)


# -- softmax_site_noise -------------------------------------------------------------------------------------------------------------
def test_noise_statistics_and_seeds():
    from vargp_amd import ops
    e = ops.softmax_site_noise(11, 10, 10, 10000, device=DEV).double().flatten()
    n = e.numel()
    assert n == 10 ** 6
    assert abs(e.mean().item()) < 5 / n ** 0.5 and abs(e.var().item() - 1) < 5 * (2 / n) ** 0.5
    a, b = ops.softmax_site_noise(11, 2, 6, 50, device=DEV), ops.softmax_site_noise(12, 2, 6, 50, device=DEV)
    assert (a - b).abs().max().item() > 1.0
    assert torch.equal(a, ops.softmax_site_noise(11, 2, 6, 50, device=DEV))


def _numpy_noise(seed, F, C, N):
    """The stream restated with test_hip_rng's numpy Philox: the draws of (n, f) are the groups (n F + f) ceil(C / 4) + j, element l
    of group j for class 4 j + l -- so element (n, f, c) of the layout (N, F, 4 ceil(C / 4)) is stream element number
    4 ((n F + f) ceil(C / 4)) + c."""
    nq = (C + 3) // 4
    flat = _normal_ref(seed, NOISE_STREAM, 0, N * F * nq * 4, 0).reshape(N, F, nq * 4)[:, :, :C]
    return torch.from_numpy(np.ascontiguousarray(flat.transpose(1, 2, 0)))          # (F, C, N) float64


@pytest.mark.parametrize('C', [6, 17])
def test_noise_is_the_documented_philox_stream(C):
    from vargp_amd import ops
    seed, F, N = 0x1234_5678_9ABC_DEF1, 3, 70
    got = ops.softmax_site_noise(seed, F, C, N, device=DEV).cpu().double()
    assert torch.allclose(got, _numpy_noise(seed, F, C, N), rtol=0, atol=2e-5)


# -- gram_moments_v -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [(130, 1000, 40, 1, 0, 'rand'), (33, 64, 32, 1, 3, 'zeros')], ids=lambda c: '-'.join(map(str, c)))
def test_gram_moments_v(case):
    """Two of test_hip_collapsed.MOMENT_CASES (two row panels, two chunks, the slab form | the direct form, a Matern epilogue, zero
    weights): with v = w * y, Phi and c are bitwise gram_moments'; with an independent v, against fp64 under the rule with
    gram_moments' own error on the same problem as the yardstick."""
    from vargp_amd import ops
    Mt, N, D, Gc, nu2, wmode = case
    theta, Z, X, w, y, _ = _moment_problem(Mt, N, D, Gc, wmode, seed=Mt + 7 * N + 13 * D)
    base = [t.cpu() for t in ops.gram_moments(_dev(theta), _dev(Z), _dev(X), _dev(w), _dev(y), nu2)]
    same = [t.cpu() for t in ops.gram_moments_v(_dev(theta), _dev(Z), _dev(X), _dev(w), _dev(w * y), nu2)]
    assert torch.equal(base[0], same[0]) and torch.equal(base[1], same[1])
    g = torch.Generator().manual_seed(9)
    v = (w * y)[:, torch.randperm(N, generator=g)].contiguous()                      # independent of w and y, of w y's scale
    got = [t.cpu() for t in ops.gram_moments_v(_dev(theta), _dev(Z), _dev(X), _dev(w), _dev(v), nu2)]
    again = [t.cpu() for t in ops.gram_moments_v(_dev(theta), _dev(Z), _dev(X), _dev(w), _dev(v), nu2)]
    assert all(torch.equal(a, b) for a, b in zip(got, again)) and torch.equal(got[0], base[0])
    rPhi, rc, _ = ref_moments(theta, Z, X, w, y, nu2)
    K = ref_kernel(Z.to(F64), X.to(F64).unsqueeze(0), theta.to(F64), nu2)
    rcv = (K * v.to(F64).unsqueeze(-2)).sum(-1)
    ec, ef = (base[1].double() - rc).abs().max().item(), (got[1].double() - rcv).abs().max().item()
    floor = float(torch.finfo(torch.float32).eps) * rcv.abs().max().item()
    print(f'{case} c: gram_moments_v {ef:.3e} gram_moments {ec:.3e} floor {floor:.3e}')
    assert ef <= max(4.0 * ec, floor)
    rs = torch.stack([w.double().sum(-1), v.double().sum(-1)], -1)
    assert torch.allclose(got[2].double(), rs, rtol=1e-6, atol=1e-5)                 # (fp64 sums of fp32 values, rounded once)


# -- fit_q_softmax_ -----------------------------------------------------------------------------------------------------------------
C_FIT, N_FIT, D_FIT, F_FIT, NOISE_SEED = 3, 300, 2, 32, 17
# data seeds for which the restatement, on the numpy restatement of the device's noise stream, takes every decision of the first 4
# iterations with a relative margin >= 1e-3: name -> seed
FIT_SEEDS = {'first': 41, 'prev': 42, 'matern': 43, 'big': 44}
# a later task's blobs are turned against the first task's: on the same blobs p(u_t | u_<) already explains the data, the fit is
# over after one step and nothing is decided by a margin
FIT_TURN = {'first': 0.0, 'prev': 0.5, 'matern': 0.0, 'big': 0.5}
# ... and with 130 + 130 inducing points even the turned blobs are fitted so fast that the fourth step gains 2.6e-4 (seeds 44 and
# 52 alike): that task's blobs lie further out, where the first task left no inducing points (smallest margin 4.5e-3)
FIT_RADIUS = {'first': 4.0, 'prev': 4.0, 'matern': 4.0, 'big': 6.0}
MARGIN = 1e-3


def _fit_inputs(name, M, kernel='rbf', prev=None):
    """The CPU side of a fit test: blobs, inducing points at random data points, a model.  -> (gp on the host, x, y)"""
    from vargp_amd.kernels import MaternKernel, RBFKernel
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.vargp import VARGP
    seed = FIT_SEEDS[name]
    x, y = blobs(C_FIT, N_FIT, D_FIT, seed, radius=FIT_RADIUS[name], turn=FIT_TURN[name])
    g = torch.Generator().manual_seed(seed + 1000)
    z = torch.stack([x[torch.randperm(N_FIT, generator=g)[:M]] for _ in range(C_FIT)])
    torch.manual_seed(seed)
    kern = RBFKernel(D_FIT, map_est=True) if kernel == 'rbf' else MaternKernel(D_FIT, nu=1.5, map_est=True)
    with torch.no_grad():
        kern.log_mean[:D_FIT] = math.log(1.5)
    gp = VARGP(z, kern, MulticlassSoftmax(n_f=10), n_var_samples=1, prev_params=[dict(p) for p in (prev or [])])
    return gp, x, y


def _restate(gp, x, y, prev, eps, nu2, n_iters):
    M, C = gp.M, gp.z.shape[0]
    theta = gp.kernel.log_mean.detach().cpu()
    z_all = torch.cat([p['z'].cpu() for p in prev] + [gp.z.detach().cpu()], -2)
    rprev = [dict(u_mean=p['u_mean'].cpu(), u_tril=ref_vec2tril(p['u_tril_vec'].cpu(), p['z'].shape[-2])) for p in prev]
    L_tt = ref_whiten(theta, z_all, rprev, nu2)[0][:, -M:, -M:]                      # start = 'prior': a_t = 0, H_t = T_tt L_tt = I
    return ref_softmax_newton(theta, z_all, rprev, x, y, None, nu2, torch.zeros(C, M, 1), L_tt, eps, n_iters=n_iters)


def _decisions(bounds):
    """The accept / reject sequence from every bound the fit evaluated, in order (the first is the starting q's)."""
    cur, out = bounds[0], []
    for b in bounds[1:]:
        ok = bool(b >= cur)
        out.append(ok)
        cur = b if ok else cur
    return out


def _fit_and_check(name, M, monkeypatch, kernel='rbf', prev=None, expect_route='fused'):
    from vargp_amd import ops, sites
    prev = prev or []
    nu2 = 0 if kernel == 'rbf' else 3
    gp, x, y = _fit_inputs(name, M, kernel, prev)
    gp = gp.to(DEV)
    eps = ops.softmax_site_noise(NOISE_SEED, F_FIT, C_FIT, N_FIT, device=DEV).cpu()
    ref = _restate(gp, x, y, prev, eps, nu2, 4)
    margins = [abs(m) for _, m in ref['decisions']]
    print(f'{name}: restatement decisions {[ok for ok, _ in ref["decisions"]]} smallest margin {min(margins):.3e} '
          f'trace {ref["trace"].view(-1).tolist()}')
    assert ref['n_iters'] == 4 and min(margins) >= MARGIN, (name, ref['decisions'])
    seen = []
    inner = sites._SoftmaxProblem.bound
    monkeypatch.setattr(sites._SoftmaxProblem, 'bound', lambda self, data, kl: seen.append(inner(self, data, kl)) or seen[-1])
    state0 = gp.u_mean.detach().clone(), gp.u_tril_vec.detach().clone()
    out = {}
    for route in dict.fromkeys(('composed', expect_route)):
        with torch.no_grad():
            gp.u_mean.copy_(state0[0])
            gp.u_tril_vec.copy_(state0[1])
        del seen[:]
        fit = gp.fit_q_softmax_(x.to(DEV), y.to(DEV), n_iters=4, start='prior', n_f=F_FIT, seed=NOISE_SEED,
                                route=None if route == expect_route else route)
        assert fit.route == route and fit.n_clamped == 0
        tr = fit.bound
        assert tr.dtype == torch.float64 and tuple(tr.shape) == (fit.n_iters + 1, 1)
        assert bool((tr[1:] >= tr[:-1]).all())
        seq = _decisions([b.cpu().item() for b in seen])
        assert seq == [ok for ok, _ in ref['decisions']], (route, seq, ref['decisions'])
        assert fit.n_iters == ref['n_iters'] and fit.n_rejected == ref['n_rejected']
        Lu = ref_vec2tril(gp.u_tril_vec.detach().cpu(), M).double()
        out[route] = dict(fit=fit, u_mean=gp.u_mean.detach().cpu().squeeze(-1).double(), S_u=Lu @ Lu.mT)
        print(f'{name} {route}: accepted {fit.n_iters} rejected {fit.n_rejected} trace {tr.view(-1).tolist()}')
    if expect_route != 'composed':
        f, c = out[expect_route], out['composed']
        _hold('u_mean', name, f['u_mean'], c['u_mean'], ref['u_mean'])
        _hold('S_u', name, f['S_u'], c['S_u'], ref['S_u'])
        _hold('trace', name, f['fit'].bound, c['fit'].bound, ref['trace'])
    return gp, out, ref


def test_fit_first_task(monkeypatch):
    _fit_and_check('first', 20, monkeypatch)


def test_fit_with_one_previous_task(monkeypatch):
    gp0, _, _ = _fit_and_check('first', 20, monkeypatch)
    prev = [dict(z=gp0.z.detach().clone(), u_mean=gp0.u_mean.detach().clone(), u_tril_vec=gp0.u_tril_vec.detach().clone())]
    gp, _, _ = _fit_and_check('prev', 20, monkeypatch, prev=prev)
    assert gp.z.shape[-2] == 20 and sum(p['z'].shape[-2] for p in prev) + 20 == 40


def test_fit_matern(monkeypatch):
    _fit_and_check('matern', 20, monkeypatch, kernel='matern')


def test_above_the_lds_limit_takes_the_composed_route(monkeypatch):
    """M = 130 and a previous task of 130: Mt = 260 > ops.SITE_MAX_MT, so the default route is the composed one; the restatement's
    decisions, and its trace to 1e-3 relative (tests/test_hip_sites.py gives the reason: the fp32 factorisation of a 260 x 260
    kernel matrix of condition number ~1e6 carries the KL term's log-determinant to about 1e-3 relative)."""
    from vargp_amd import ops
    assert 260 > ops.SITE_MAX_MT
    gp0, x0, y0 = _fit_inputs('first', 130)
    gp0 = gp0.to(DEV)
    gp0.fit_q_softmax_(x0.to(DEV), y0.to(DEV), n_iters=4, start='prior', n_f=F_FIT, seed=NOISE_SEED)
    prev = [dict(z=gp0.z.detach().clone(), u_mean=gp0.u_mean.detach().clone(), u_tril_vec=gp0.u_tril_vec.detach().clone())]
    _, out, ref = _fit_and_check('big', 130, monkeypatch, prev=prev, expect_route='composed')
    got = out['composed']['fit'].bound
    assert torch.allclose(got, ref['trace'], rtol=1e-3, atol=0.0), (got, ref['trace'])


def test_full_fit_trace_never_falls_and_predict_accepts_q():
    gp, x, y = _fit_inputs('first', 20)
    gp = gp.to(DEV)
    fit = gp.fit_q_softmax_(x.to(DEV), y.to(DEV), n_iters=20, start='prior', n_f=F_FIT, seed=NOISE_SEED)
    tr = fit.bound
    print(f'full fit: accepted {fit.n_iters} rejected {fit.n_rejected} trace {tr.view(-1).tolist()}')
    assert tuple(tr.shape) == (fit.n_iters + 1, 1) and fit.n_iters >= 4 and bool((tr[1:] >= tr[:-1]).all())
    assert fit.n_clamped == 0 and fit.route == 'fused'
    with torch.no_grad():
        probs = gp.predict(x.to(DEV)).cpu()
    assert tuple(probs.shape) == (N_FIT, C_FIT) and bool(torch.isfinite(probs).all())
    assert torch.allclose(probs.sum(-1), torch.ones(N_FIT), atol=1e-4)
    assert (probs.argmax(-1) == y).double().mean().item() >= 0.95    # (the blobs overlap in well under 1 % of the points)


# -- end to end ---------------------------------------------------------------------------------------------------------------------
def test_create_clf_q_init_newton_softmax():
    """The same factory call with and without q_init='newton_softmax' (same seed: same inducing points): the training accuracy of
    gp.predict is at least the accuracy of the restatement's converged q (same model, the device's site noise, the same
    prediction draws) minus 0.02, and the nll term of the loss is lower than the default start's."""
    from vargp_amd import noise, ops
    from vargp_amd.vargp import VARGP
    x, y = blobs(C_FIT, N_FIT, D_FIT, 51)
    data = _Data(x, y)
    make = lambda **kw: VARGP.create_clf(data, M=20, n_f=10, n_var_samples=1, map_est_hypers=True, **kw)
    models = {}
    for q_init in ('default', 'newton_softmax'):
        torch.manual_seed(5)
        models[q_init] = make(q_init=q_init, newton_iters=20, site_samples=F_FIT) if q_init != 'default' else make()
        assert models[q_init].z.device.type == 'cpu'
    a, b = models['default'], models['newton_softmax']
    assert torch.equal(a.z, b.z) and not torch.equal(a.u_mean, b.u_mean) and not torch.equal(a.u_tril_vec, b.u_tril_vec)
    eps = ops.softmax_site_noise(0, F_FIT, C_FIT, N_FIT, device=DEV).cpu()         # (the factory fits with the default seed 0)
    ref = _restate(b, x, y, [], eps, 0, 20)
    # both sides predict by the model's own rule, the mean over n_f draws of softmax(mu + sqrt(var) eps_f), on the SAME draws: with
    # the factory's lengthscale of 0.5 a class's inducing points cover its own blob alone, the other classes' latents are N(0, 1)
    # there, and ten draws of them flip some predictions whatever q(u) is
    g = torch.Generator().manual_seed(6)
    eps_f = torch.randn(1, 10, C_FIT, N_FIT, generator=g)
    p_ref = torch.softmax(ref['mu'] + ref['var'].sqrt() * eps_f[0].double(), -2).mean(0)
    ref_acc = (p_ref.argmax(0) == y).double().mean().item()
    nll = {}
    for k, gp in models.items():
        gp = gp.to(DEV)
        with torch.no_grad(), noise.inject(eps_f=eps_f.to(DEV)):
            nll[k] = float(gp.loss(x.to(DEV), y.to(DEV))[2])
            acc = (gp.predict(x.to(DEV)).cpu().argmax(-1) == y).double().mean().item()
        print(f'{k}: nll {nll[k]:.4f} accuracy {acc:.4f} (restatement {ref_acc:.4f})')
    assert acc >= ref_acc - 0.02
    assert nll['newton_softmax'] < nll['default']
