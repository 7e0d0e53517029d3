"""The leave-one-out cavity on the device: ops.site_cavity and ops.site_marginals_s (csrc/sites.hip: vargp_site_cavity), VARGP.loo
(vargp_amd/loo.py), against the fp64 restatement of tests/test_loo_host.py.

Rule (tests/test_hip_sites.py's, unchanged): no tolerance is fixed in advance.  For each checked quantity the error of the COMPOSED
route (loo.composed_site_cavity / composed_marginals_s: the per-op fp32 kernels, the cavity arithmetic in fp64 torch) against the
fp64 restatement is measured on the same inputs, and the fused kernel may be at most 4 x that, with an absolute floor of one fp32
ulp of the largest entry of the quantity.  Errors are max-abs.  Every kernel-level case asserts from the restatement that
min r_n >= 0.5 (V is rescaled where a seed violates it), which keeps 1 / r from amplifying the error.

Composed-route errors against fp64 (max-abs over the three outputs), as test_site_cavity_against_fp64 printed them on an MI355X
(Mv = Mt):
#  case (Mt, N, D, nu2, kind, shared y, w)            s         mu_c      var_c     lam1      lam2
#  (1, 1, 1, 0, probit, per-output, None)             5.3e-09   5.5e-09   1.1e-07   9.7e-08   7.3e-08
#  (63, 63, 32, 1, logit, shared, None)               3.7e-08   4.2e-08   7.6e-08   1.1e-07   4.6e-08
#  (64, 65, 33, 3, poisson, per-output, zeros)        6.1e-08   2.2e-07   1.2e-07   2.8e-07   1.4e-07
#  (65, 513, 40, 5, studentt, per-output, None)       7.1e-08   9.1e-08   1.1e-07   6.5e-08   1.0e-07
#  (130, 513, 32, 0, studentt, shared, rand)          3.9e-08   9.5e-08   1.2e-07   9.4e-08   1.4e-07
#  (200, 65, 33, 3, probit, shared, rand)             9.8e-08   2.1e-07   1.5e-07   2.2e-07   2.0e-07
# (the fused kernel's largest error over all cases and quantities was 2.0 x the composed route's.)
# VARGP.loo (M = 20, D = 2, N = 300), composed route against the restatement at the fitted q (mu, var, lpd):
#  Gaussian C = 2 after fit_q_: first task 3.1e-06, 1.4e-05, 1.8e-04; with a previous task 9.7e-06, 5.9e-05, 6.2e-04
#  probit C = 2 after fit_q_newton_: first task 2.3e-06, 3.1e-06, 3.9e-06; with a previous task 3.4e-06, 4.4e-06, 3.4e-06
#  softmax C = 3 after fit_q_softmax_ (moments only): 3.0e-06, 1.2e-06
#  stationarity after a converged fit_q_ (both routes run the same moment pass): [1.1e-04, 4.2e-06]
#  Mt = 260 (composed route only), max-abs error of mu, var, lpd: 6.3e-06 of 1.4, 9.7e-06 of 0.24, 6.4e-06 of 2.5
"""
import math

import pytest
import torch

from test_collapsed import ref_vec2tril, ref_whiten
from test_hip_lpd import lp_terms
from test_hip_sites import DF, G, KIND, _dev, _extra, _hold, _model, _site_problem
from test_loo_host import F64, ref_cavity, ref_cavity_ops

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (Mt, N, D, nu2, kind, shared targets, weights): test_hip_sites.SITE_CASES' reasons -- Mt on both sides of one, two and three
# 64-row panels (V has as many column panels, and 1 to 4 row panels), N around the 64-column step and over two chunks, D on both
# sides of kRbfDirectD = 32, every kind and every epilogue
CAVITY_CASES = [
    (1, 1, 1, 0, 'probit', False, None),
    (63, 63, 32, 1, 'logit', True, None),
    (64, 65, 33, 3, 'poisson', False, 'zeros'),
    (65, 513, 40, 5, 'studentt', False, None),
    (130, 513, 32, 0, 'studentt', True, 'rand'),
    (200, 65, 33, 3, 'probit', True, 'rand'),
]


def _mvs(Mt):
    return sorted({1, Mt} | ({Mt - 37} if Mt > 37 else set()))


def _cavity_problem(Mt, N, D, kind, shared, wmode, Mv, seed, nu2, target=None):
    """test_hip_sites._site_problem with V = 0.3 randn / sqrt(Mt) (G, Mv, Mt).  target None: V is scaled down if the restatement's
    min r_n is below 0.5; else V is scaled so that max lam2_n s_n = target.  -> (problem, restatement)"""
    pr = _site_problem(Mt, N, D, kind, shared, wmode, seed)
    g = torch.Generator().manual_seed(seed + 7)
    pr['V'] = 0.3 * torch.randn(G, Mv, Mt, generator=g) / math.sqrt(Mt)
    restate = lambda: ref_cavity_ops(kind, pr['par'], pr['theta'], pr['Z'], pr['X'], pr['alpha'], pr['Q'], pr['V'], pr['y'], pr['w'], nu2)
    ref = restate()
    top = (ref['lam2'] * ref['s']).max().item()
    if target is not None or top > 0.5:
        pr['V'] = (pr['V'].double() * math.sqrt((0.45 if target is None else target) / top)).float()
        ref = restate()
    return pr, ref


def _call(fn, pr, kind, nu2, with_targets=True):
    okind, extra = _extra(kind, pr['log_scale'])
    args = [_dev(pr[k]) for k in ('theta', 'Z', 'X', 'alpha', 'Q', 'V')]
    out = fn(*args, _dev(pr['y']), _dev(pr['w']), okind, extra, nu2) if with_targets else fn(*args, nu2)
    torch.cuda.synchronize()
    return out.__class__(*(t.cpu() for t in out)) if hasattr(out, '_fields') else tuple(t.cpu() for t in out)


@pytest.mark.parametrize('case', CAVITY_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_site_cavity_against_fp64(case):
    from vargp_amd import loo, ops
    Mt, N, D, nu2, kind, shared, wmode = case
    if N == 513:
        assert ops.site_cavity_chunks(G, Mt, N, D) >= 2
    for Mv in _mvs(Mt):
        pr, ref = _cavity_problem(Mt, N, D, kind, shared, wmode, Mv, 100 + Mt + N + D, nu2)
        tag = f'{case} Mv={Mv}'
        on = torch.ones_like(ref['r'], dtype=torch.bool) if pr['w'] is None else pr['w'] != 0
        print(f'{tag}: min r {ref["r"][on].min().item():.3f}, max s {ref["s"].max().item():.3e}')
        assert ref['r'][on].min().item() >= 0.5 and int(ref['n_unstable'].sum()) == 0
        comp = _call(loo.composed_site_cavity, pr, kind, nu2)
        fused = _call(ops.site_cavity, pr, kind, nu2)
        assert all(bool(torch.isfinite(t).all()) for t in fused)
        for name in ('mu', 'var', 's', 'lam1', 'lam2', 'mu_c', 'var_c'):
            _hold(name, tag, getattr(fused, name), getattr(comp, name), ref[name])
        assert fused.n_unstable.dtype == torch.int64 and fused.n_unstable.tolist() == [0] * G == comp.n_unstable.tolist()
        # the marginals form: the same three arrays, against its own composed route
        mc, mf = _call(loo.composed_marginals_s, pr, kind, nu2, False), _call(ops.site_marginals_s, pr, kind, nu2, False)
        for name, f, c in zip(('mu', 'var', 's'), mf, mc):
            _hold(name + ' (marginals form)', tag, f, c, ref[name])
        if wmode == 'zeros':
            off = pr['w'] == 0
            assert torch.equal(fused.mu_c[off], fused.mu[off]) and torch.equal(fused.var_c[off], fused.var[off])
            assert bool((fused.lam1[off] == 0).all()) and bool((fused.lam2[off] == 0).all())


def test_unstable_points_are_nan_and_counted():
    """V scaled so that max lam2_n s_n = 1.5: the points with lam2_n s_n >= 1 are unstable ([41, 3, 4] of 513, over two chunks).  The restatement defines the set (its
    |r_n| stays above 1e-3, so fp32 cannot move a point across); the counts are equal, NaN sits exactly there and nowhere else."""
    from vargp_amd import loo, ops
    Mt, N, D, nu2, kind = 130, 513, 40, 0, 'logit'
    pr, ref = _cavity_problem(Mt, N, D, kind, False, 'rand', 93, 5, nu2, target=1.5)
    bad = ref['unstable']
    print(f'unstable {ref["n_unstable"].tolist()} of {N}; min |r| {ref["r"].abs().min().item():.2e}')
    assert ref['r'].abs().min().item() > 1e-3 and bool((ref['n_unstable'] > 0).all()) and bool((ref['n_unstable'] < N).all())
    for fn in (ops.site_cavity, loo.composed_site_cavity):
        out = _call(fn, pr, kind, nu2)
        assert torch.equal(out.n_unstable, ref['n_unstable'])
        assert torch.equal(torch.isnan(out.mu_c), bad) and torch.equal(torch.isnan(out.var_c), bad)
        assert all(bool(torch.isfinite(t).all()) for t in (out.mu, out.var, out.s, out.lam1, out.lam2))


def test_zero_weight_points_keep_their_marginals_bitwise():
    from vargp_amd import ops
    for kind, D in (('poisson', 33), ('studentt', 2)):
        pr, _ = _cavity_problem(65, 300, D, kind, False, 'zeros', 28, 7, 0)
        off = pr['w'] == 0
        assert 0 < int(off.sum()) < off.numel()
        pr['y'][off] = 1e4                                            # (a target no likelihood could digest: it is never read)
        out = _call(ops.site_cavity, pr, kind, 0)
        assert torch.equal(out.mu_c[off], out.mu[off]) and torch.equal(out.var_c[off], out.var[off])
        assert bool((out.lam1[off] == 0).all()) and bool((out.lam2[off] == 0).all()) and out.n_unstable.tolist() == [0] * G
        assert not torch.equal(out.mu_c[~off], out.mu[~off])


def test_two_calls_are_bitwise_equal():
    from vargp_amd import ops
    pr, _ = _cavity_problem(130, 513, 40, 'logit', False, 'rand', 93, 9, 3)
    a, b = _call(ops.site_cavity, pr, 'logit', 3), _call(ops.site_cavity, pr, 'logit', 3)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    a, b = _call(ops.site_marginals_s, pr, 'logit', 3, False), _call(ops.site_marginals_s, pr, 'logit', 3, False)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_cavity_entry_rejects_before_any_launch():
    """The export resolves; Mt > 256, Mv > Mt and a null pointer are VARGP_EINVAL with DEVICE operands too: nothing is launched."""
    import ctypes
    from vargp_amd._lib import lib, ptr, stream_ptr
    L = lib()
    assert hasattr(L, 'vargp_site_cavity')
    t = torch.zeros(1 << 20, device=DEV)
    p, null = ptr(t), ctypes.c_void_p(0)

    def call(ins=None, dims=(1, 5, 3, 9, 2), kind=-1):
        return L.vargp_site_cavity(*(ins or [p] * 6), p, 9, p, kind, p, 4.0, 0.0, *([p] * 8), *dims, 0, p, t.numel() * 4, stream_ptr())

    assert call(dims=(1, 257, 3, 9, 2)) == -1 and call(dims=(1, 257, 3, 9, 2), kind=0) == -1
    assert call(dims=(1, 5, 6, 9, 2)) == -1 and call(dims=(1, 5, 6, 9, 2), kind=2) == -1
    assert call(ins=[p] * 5 + [null]) == -1 and call(ins=[null] + [p] * 5, kind=0) == -1
    assert b'site_cavity' in L.vargp_last_error()
    torch.cuda.synchronize()
    assert float(t.abs().sum()) == 0.0


# -- VARGP.loo ----------------------------------------------------------------------------------------------------------------------
def _gauss_model(C, M, D, N, seed, prev=None):
    from vargp_amd.kernels import RBFKernel
    from vargp_amd.likelihoods import GaussianLikelihood
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, D, generator=g)
    y = torch.stack([torch.sin(1.5 * x[:, 0] + c) + 0.3 * x[:, -1] for c in range(C)]) + 0.2 * torch.randn(C, N, generator=g)
    z = torch.stack([x[torch.randperm(N, generator=g)[:M]] for _ in range(C)])
    torch.manual_seed(seed)
    gp = VARGP(z, RBFKernel(D, map_est=True), GaussianLikelihood(C, init_log_var=-3.0), n_var_samples=1, prev_params=prev).to(DEV)
    return gp, x, y


def _restate(gp, kind, par, x, y, prev, eps=None):
    """ref_cavity at the model's current parameters and q(u_t), all read back to the host."""
    M = gp.M
    theta = gp.kernel.log_mean.detach().cpu()
    z_all = torch.cat([p['z'].cpu() for p in prev] + [gp.z.detach().cpu()], -2)
    rprev = [dict(u_mean=p['u_mean'].cpu(), u_tril=ref_vec2tril(p['u_tril_vec'].cpu(), p['z'].shape[-2])) for p in prev]
    T_tt = ref_whiten(theta, z_all, rprev, 0)[1][:, -M:, -M:]
    a_t = (T_tt @ gp.u_mean.detach().cpu().double()).squeeze(-1)
    H_t = T_tt @ ref_vec2tril(gp.u_tril_vec.detach().cpu(), M).double()
    return ref_cavity(kind, par, theta, z_all, rprev, x, y, None, 0, a_t, H_t, eps)


def _params(gp):
    return dict(z=gp.z.detach().clone(), u_mean=gp.u_mean.detach().clone(), u_tril_vec=gp.u_tril_vec.detach().clone())


def _both_routes(gp, x, y, **kw):
    out = {}
    for route in ('composed', 'fused'):
        res = gp.loo(x.to(DEV), y.to(DEV), route=None if route == 'fused' else route, **kw)
        torch.cuda.synchronize()
        assert res.route == route and res.n_unstable.tolist() == [0] * gp.z.shape[0]
        assert tuple(res.lpd.shape) == (x.shape[0],) and tuple(res.mu.shape) == tuple(res.var.shape) == (gp.z.shape[0], x.shape[0])
        out[route] = res
    return out['fused'], out['composed']


def _check_loo(tag, lik, par, gp, x, y, prev):
    kind = 'gauss' if lik == 'gaussian' else lik
    rpar = dict(beta=(-par.double()).exp()) if lik == 'gaussian' else {}
    ref = _restate(gp, kind, rpar, x, y, prev)
    assert int(ref['n_unstable'].sum()) == 0
    f, c = _both_routes(gp, x, y)
    lp = lp_terms(lik, ref['mu_c'].unsqueeze(0), ref['var_c'].unsqueeze(0), y, None if par is None else par.double())[0]
    _hold('mu', tag, f.mu.cpu(), c.mu.cpu(), ref['mu_c'])
    _hold('var', tag, f.var.cpu(), c.var.cpu(), ref['var_c'])
    _hold('lpd', tag, f.lpd.cpu(), c.lpd.cpu(), lp.sum(0))
    _hold('lpd_out', tag, f.lpd_out.cpu(), c.lpd_out.cpu(), lp)
    print(f'{tag}: mean loo lpd {f.lpd.mean().item():.4f}; min r {ref["r"].min().item():.3f}')
    return f, c


def test_loo_gaussian_first_task_and_with_a_previous_task():
    """After fit_q_ (the fixed point: exact LOO); check=True: the fused route's stationarity is below 4 x the composed one's."""
    gp0, x, y = _gauss_model(2, 20, 2, 300, 22)
    gp0.fit_q_(x.to(DEV), y.to(DEV))
    par = gp0.likelihood.obs_log_var.detach().cpu()
    _check_loo('gauss first', 'gaussian', par, gp0, x, y, [])
    st = {r: gp0.loo(x.to(DEV), y.to(DEV), route=r, check=True).stationarity.cpu() for r in ('fused', 'composed')}
    print(f'stationarity after fit_q_: fused {st["fused"].tolist()} composed {st["composed"].tolist()}')
    assert st['fused'].dtype == torch.float64 and tuple(st['fused'].shape) == (2,)
    assert bool((st['fused'] < 4.0 * st['composed']).all())
    prev = [_params(gp0)]
    gp1, x1, y1 = _gauss_model(2, 20, 2, 300, 23, prev=[dict(p) for p in prev])
    gp1.fit_q_(x1.to(DEV), y1.to(DEV))
    _check_loo('gauss prev', 'gaussian', par, gp1, x1, y1, prev)


def test_loo_probit_first_task_and_with_a_previous_task():
    gp0, x, y = _model('probit', 2, 20, 2, 300, 22)
    gp0.fit_q_newton_(x.to(DEV), y.to(DEV))
    _check_loo('probit first', 'probit', None, gp0, x, y, [])
    prev = [_params(gp0)]
    gp1, x1, y1 = _model('probit', 2, 20, 2, 300, 23, prev=[dict(p) for p in prev])
    gp1.fit_q_newton_(x1.to(DEV), y1.to(DEV))
    _check_loo('probit prev', 'probit', None, gp1, x1, y1, prev)


def test_loo_softmax_moments_and_lpd():
    """C = 3 after fit_q_softmax_: the cavity moments against the restatement on the same noise (ops.softmax_site_noise); the lpd
    draws its own noise, so it is compared with likelihood.log_prob on the returned moments under the same noise.inject."""
    from vargp_amd import noise, ops
    from test_hip_softmax_sites import C_FIT, F_FIT, N_FIT, NOISE_SEED, _fit_inputs
    gp, x, y = _fit_inputs('first', 20)
    gp = gp.to(DEV)
    gp.fit_q_softmax_(x.to(DEV), y.to(DEV), n_iters=4, start='prior', n_f=F_FIT, seed=NOISE_SEED)
    eps = ops.softmax_site_noise(NOISE_SEED, F_FIT, C_FIT, N_FIT, device=DEV).cpu()
    ref = _restate(gp, 'softmax', {}, x, y, [], eps)
    assert int(ref['n_unstable'].sum()) == 0
    eps_f = torch.randn(1, gp.likelihood.n_f, C_FIT, N_FIT, generator=torch.Generator().manual_seed(3)).to(DEV)
    with noise.inject(eps_f=eps_f):
        f, c = _both_routes(gp, x, y, n_f=F_FIT, seed=NOISE_SEED)
        want = gp.likelihood.log_prob(f.mu.unsqueeze(0).contiguous(), f.var.unsqueeze(0).contiguous(), y.to(DEV))
    _hold('mu', 'softmax', f.mu.cpu(), c.mu.cpu(), ref['mu_c'])
    _hold('var', 'softmax', f.var.cpu(), c.var.cpu(), ref['var_c'])
    assert f.lpd_out is None and torch.equal(f.lpd, want) and bool(torch.isfinite(f.lpd).all())
    print(f'softmax: mean loo lpd {f.lpd.mean().item():.4f}; min r {ref["r"].min().item():.3f}')


def test_above_the_lds_limit_takes_the_composed_route():
    """Mt = 260 > ops.SITE_MAX_MT: the default route is the composed one, and it agrees with the restatement to the rtol of
    test_hip_sites.test_above_the_lds_limit_takes_the_composed_route (1e-3; atol: that fraction of the largest entry)."""
    from vargp_amd import ops
    assert 260 > ops.SITE_MAX_MT
    gp, x, y = _model('probit', 1, 260, 2, 300, 24)
    gp.fit_q_newton_(x.to(DEV), y.to(DEV))
    res = gp.loo(x.to(DEV), y.to(DEV))
    assert res.route == 'composed' and res.n_unstable.tolist() == [0]
    with pytest.raises(ValueError, match=str(ops.SITE_MAX_MT)):
        gp.loo(x.to(DEV), y.to(DEV), route='fused')
    ref = _restate(gp, 'probit', {}, x, y, [])
    lp = lp_terms('probit', ref['mu_c'].unsqueeze(0), ref['var_c'].unsqueeze(0), y, None)[0].sum(0)
    for name, got, want in (('mu', res.mu, ref['mu_c']), ('var', res.var, ref['var_c']), ('lpd', res.lpd, lp)):
        err = (got.cpu().double() - want).abs().max().item()
        print(f'Mt = 260 {name}: max-abs error {err:.3e} of {want.abs().max().item():.3e}')
        assert torch.allclose(got.cpu().double(), want, rtol=1e-3, atol=1e-3 * want.abs().max().item()), name


def test_compute_loo_is_the_mean_over_the_stable_points():
    """train_utils.compute_loo on a data set with (C,) target vectors: the mean of VARGP.loo's lpd, none unstable after fit_q_; and
    with q(u_t) made three times as wide as the fixed point, the unstable points are counted and left out of the mean."""
    from test_collapsed import _Data
    from vargp_amd.train_utils import compute_loo
    gp, x, y = _gauss_model(2, 20, 2, 300, 22)
    gp.fit_q_(x.to(DEV), y.to(DEV))
    data = _Data(x, y.t().contiguous())
    mean, n_unstable = compute_loo(data, gp, device=DEV)
    res = gp.loo(x.to(DEV), y.to(DEV))
    assert n_unstable == 0 and mean == pytest.approx(res.lpd.double().mean().item(), rel=1e-12)
    with torch.no_grad():
        gp.u_tril_vec.copy_(mat2vec_scaled(gp, 3.0))
    res = gp.loo(x.to(DEV), y.to(DEV))
    bad = torch.isnan(res.lpd)
    mean, n_unstable = compute_loo(data, gp, device=DEV)
    print(f'u_tril x 3: {int(bad.sum())} of 300 points unstable, per output {res.n_unstable.tolist()}; mean over the rest {mean:.4f}')
    assert 0 < int(bad.sum()) < 300 and n_unstable == int(bad.sum()) and int(res.n_unstable.sum()) >= n_unstable
    assert torch.equal(bad, torch.isnan(res.mu).any(0)) and mean == pytest.approx(res.lpd[~bad].double().mean().item(), rel=1e-12)


def mat2vec_scaled(gp, factor):
    """u_tril_vec of factor x the model's u_tril (the diagonal goes through the inverse softplus of vec2tril)."""
    from vargp_amd import ops
    from vargp_amd.whitened import inv_softplus
    vec = ops.mat2trilvec(factor * ops.vec2tril(gp.u_tril_vec.detach().float(), gp.M))
    idx = torch.arange(gp.M, device=vec.device)
    diag = idx * (idx + 1) // 2 + idx
    vec[:, diag] = inv_softplus(vec[:, diag].double()).float()
    return vec
