"""The differentiable softmax site bound on the device: ops.softmax_site_grads (csrc/softmax_sites.hip: vargp_softmax_site_grads),
ops.site_transport_bwd (csrc/sites.hip: vargp_site_transport_bwd), ops.softmax_site_bound_diff, VARGP.softmax_site_bound,
VARGP.fit_softmax_sites_ and create_clf(q_init='em_softmax'), against the fp64 restatement of
tests/test_softmax_site_bound_host.py.

Rule (that of tests/test_hip_sites.py and tests/test_hip_site_bound.py): no tolerance is fixed in advance.  For each quantity the
max-abs error of the COMPOSED route (the per-op fp32 kernels and fp32 elementwise torch: sites.softmax_value_torch,
sites._tile_marginals, sites.composed_softmax_site_bound) against the fp64 restatement is measured on the same input, and the fused
kernel may be at most 4 x that, with a floor of one fp32 ulp of the quantity's largest entry.

Composed-route errors against fp64 (max-abs), as the tests printed them on an MI355X:
#  softmax_site_grads (C, N, F, w)   gmu       gvar          site_transport_bwd (Mt, N, D, nu2)   gtheta    gZ        galpha    gQ
#  (2, 1, 1, None)                  3.1e-08   0 (var = 0)   (1, 1, 1, 0)                         1.7e-08   1.5e-09   1.7e-08   2.9e-11
#  (3, 63, 4, rand)                 1.6e-07   6.6e-08       (63, 63, 32, 1)                      4.1e-06   6.2e-09   4.8e-07   1.5e-07
#  (10, 65, 10, zeros), +-60        6.0e-08   1.4e-30       (64, 65, 33, 3), Q x 4               1.9e-06   8.7e-09   4.7e-07   6.4e-08
#  (16, 65, 2, None)                2.5e-07   1.4e-07       (130, 513, 40, 5)                    4.2e-06   5.3e-08   5.3e-06   1.7e-06
#  (17, 513, 3, rand)               2.5e-07   3.7e-07       (256, 65, 33, 0)                     4.3e-06   9.4e-09   5.2e-07   3.9e-07
#  (33, 300, 2, zeros)              1.4e-07   2.0e-07       (65, 65, 130, 0)                     1.3e-06   3.3e-09   3.5e-07   2.1e-07
#  (128, 70, 2, None)               1.2e-07   1.0e-07
# variances that clamp in fp64 with the margin 1e-4 gamma^2: 2 of 3, 0 of 189, 159 of 195, 1 of 1539, 3 of 195, 0 of 195
#  softmax_site_bound_diff (C, Mt, N, D, F)   gtheta    gZ        galpha    gQ        value
#  (3, 1, 1, 1, 1)                            5.6e-08   7.1e-09   2.8e-08   6.9e-08   8.7e-08
#  (3, 65, 513, 33, 3)                        2.3e-06   2.5e-08   2.7e-06   1.4e-06   3.7e-06
#  (17, 256, 65, 2, 2)                        7.1e-06   1.7e-07   8.1e-07   2.8e-06   2.1e-06
# VARGP.softmax_site_bound (M = 10, D = 2, N = 300, C = 3, n_f = 32), composed route against the restatement (z, log_mean, bound):
#  first task 6.0e-05, 7.5e-05, 8.8e-07;  with a previous task 1.1e-04, 5.0e-04, 2.6e-05;  Matern 3/2 2.0e-05, 2.1e-04, 4.4e-06
# fit_softmax_sites_(n_rounds=2, m_steps=5) from the prior: trace -125.464, -113.201, -102.499; 18 Newton steps; stopped 'rounds'
"""
import math

import pytest
import torch

from test_collapsed import _Data, ref_vec2tril
from test_hip_sites import DEV, ULP32, _dev, _site_problem
from test_hip_softmax_sites import SOFTMAX_CASES, _softmax_problem
from test_softmax_site_bound_host import (EM_C, EM_D, EM_F, EM_M, EM_N, em_inputs, ref_softmax_data_term, ref_softmax_marginals,
                                          ref_softmax_site_bound, ref_softmax_value)

pytestmark = pytest.mark.gpu
F64 = torch.float64
G = 3
NOISE_SEED = 17


def _hold(name, tag, fused, comp, ref):
    """fused error <= max(4 x composed error, one fp32 ulp of the largest entry)"""
    ef, ec = (fused.double() - ref).abs().max().item(), (comp.double() - ref).abs().max().item()
    floor = ULP32 * ref.abs().max().item()
    print(f'{tag} {name}: fused {ef:.3e} composed {ec:.3e} floor {floor:.3e}')
    assert ef <= max(4.0 * ec, floor), (tag, name, ef, ec, floor)


# -- softmax_site_grads -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SOFTMAX_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_softmax_site_grads_against_fp64(case):
    """gmu and gvar at test_hip_softmax_sites' cases (C = 2, 16 | 17, 128, C % 4 != 0, N around 64 and 513, var = 0 entries, zero
    weights, mu = +-60) against the fp64 autograd of the restatement on the device's own noise."""
    from vargp_amd import ops, sites
    C, N, F, wmode = case
    seed = 1000 + C + N
    mu, var, y, w = _softmax_problem(C, N, F, wmode, seed)
    eps = ops.softmax_site_noise(seed, F, C, N, device=DEV)
    leaves = [mu.double().requires_grad_(True), var.double().requires_grad_(True)]
    ref = torch.autograd.grad(ref_softmax_value(*leaves, y, w, eps.cpu()).sum(), leaves)
    dl = [_dev(mu).requires_grad_(True), _dev(var).requires_grad_(True)]
    comp = [t.cpu() for t in torch.autograd.grad(sites.softmax_value_torch(*dl, _dev(y), _dev(w), eps), dl)]
    one = torch.ones(1, device=DEV)
    run = lambda gout=one, **kw: [t.cpu() for t in ops.softmax_site_grads(_dev(mu), _dev(var), _dev(y), _dev(w), F, gout, **kw)]
    fused = run(eps=eps)
    assert all(tuple(t.shape) == (C, N) and bool(torch.isfinite(t).all()) for t in fused)
    tag = str(case)
    _hold('gmu', tag, fused[0], comp[0], ref[0])
    _hold('gvar', tag, fused[1], comp[1], ref[1])
    assert int((var == 0).sum()) > 0 and bool((fused[1][var == 0] == 0).all())
    # the noise generated inside the kernel is the noise softmax_site_noise writes; two calls are bitwise equal
    own, again = run(seed=seed), run(seed=seed)
    for u, v, t in zip(fused, own, again):
        assert torch.equal(u, v) and torch.equal(v, t)
    # a seed other than 1 scales linearly (a power of two: exactly, but for entries in the denormal range)
    half = run(gout=torch.full((1,), -0.5, device=DEV), seed=seed)
    for u, v in zip(own, half):
        assert torch.allclose(v, -0.5 * u, rtol=1e-6, atol=1e-37)
    if wmode == 'zeros':
        off = w == 0
        assert 0 < int(off.sum()) < N and bool((fused[0][:, off] == 0).all()) and bool((fused[1][:, off] == 0).all())
        g = torch.Generator().manual_seed(5)
        mu2, var2, y2 = mu.clone(), var.clone(), y.clone()
        mu2[:, off] = 1e4 * torch.randn(C, int(off.sum()), generator=g)
        var2[:, off] = float('nan')
        y2[off] = (y[off] + 1) % C
        other = [t.cpu() for t in ops.softmax_site_grads(_dev(mu2), _dev(var2), _dev(y2), _dev(w), F, one, seed=seed)]
        for u, v in zip(own, other):
            assert torch.equal(u, v)


def test_softmax_site_grads_refuses_more_than_128_classes():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    mu = torch.zeros(129, 4, device=DEV)
    with pytest.raises(VargpHipError, match='128'):
        ops.softmax_site_grads(mu, mu, torch.zeros(4, dtype=torch.int64, device=DEV), None, 2, torch.ones(1, device=DEV))


# -- site_transport_bwd -------------------------------------------------------------------------------------------------------------
# (Mt, N, D, nu2): one row, one column; both sides of one panel and of the 64-column step, both distance forms (D <= 32 | > 32);
# two row panels over two chunks; the limit Mt = 256; two groups of d (D = 130 > 128)
TRANSPORT_CASES = [(1, 1, 1, 0), (63, 63, 32, 1), (64, 65, 33, 3), (130, 513, 40, 5), (256, 65, 33, 0), (65, 65, 130, 0)]
CLAMP_CASE, CLAMP_Q_SCALE = (64, 65, 33, 3), 4.0                  # Q scaled up until some, not all, variances clamp to exactly 0


def _transport_problem(case):
    Mt, N, D, nu2 = case
    pr = _site_problem(Mt, N, D, 'probit', True, None, seed=500 + Mt + N + D)
    if case == CLAMP_CASE:
        pr['Q'] = pr['Q'] * CLAMP_Q_SCALE
    g = torch.Generator().manual_seed(7 + Mt)
    gm, gv = torch.randn(G, N, generator=g), torch.randn(G, N, generator=g)
    off = torch.zeros(N, dtype=torch.bool)
    off[torch.randperm(N, generator=g)[:N // 3]] = True           # a third of the columns: both seeds 0 in every output
    gm[:, off], gv[:, off] = 0.0, 0.0
    return pr, gm, gv, off


def _functional(mu, var, gm, gv):
    return (gm * mu).sum() + (gv * var).sum()


def _transport(pr, gm, gv, nu2, X=None):
    from vargp_amd import ops
    out = ops.site_transport_bwd(_dev(pr['theta']), _dev(pr['Z']), _dev(pr['X'] if X is None else X), _dev(pr['alpha']), _dev(pr['Q']),
                                 _dev(gm), _dev(gv), nu2)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


@pytest.mark.parametrize('case', TRANSPORT_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_site_transport_bwd_against_fp64(case):
    """gZ, gtheta (all D + 1 entries) and galpha of the linear functional sum gm mu + sum gv var (clamp included) against its fp64
    autograd; gv_out = gv u; NaN in the rows of X of the all-zero columns changes nothing; two calls are bitwise equal."""
    from vargp_amd import ops, sites
    Mt, N, D, nu2 = case
    pr, gm, gv, off = _transport_problem(case)
    if N == 513:
        assert ops.site_transport_bwd_chunks(G, Mt, N, D) >= 2
    names = ('theta', 'Z', 'alpha', 'Q')
    leaves = [pr[k].double().requires_grad_(True) for k in names]
    mu, raw = ref_softmax_marginals(leaves[0], leaves[1], pr['X'], leaves[2], leaves[3], nu2)
    ref = torch.autograd.grad(_functional(mu, raw.clamp_min(0.0), gm.double(), gv.double()), leaves)
    dl = [_dev(pr[k]).requires_grad_(True) for k in names]
    K = sites._gram_tile(dl[0].view(1, -1), dl[1], _dev(pr['X']), nu2)
    cmu, cvar = sites._tile_marginals(K, dl[2], 0.5 * (dl[3] + dl[3].mT), (2.0 * dl[0][-1]).exp())
    comp = [t.cpu() for t in torch.autograd.grad(_functional(cmu, cvar, _dev(gm), _dev(gv)), dl)]
    fused = _transport(pr, gm, gv, nu2)
    gZ, gtheta, galpha, gv_out = fused
    assert tuple(gZ.shape) == (G, Mt, D) and tuple(gtheta.shape) == (D + 1,) and tuple(galpha.shape) == (G, Mt)
    assert all(bool(torch.isfinite(t).all()) for t in fused)
    tag = str(case)
    _hold('gtheta', tag, gtheta, comp[0], ref[0])
    _hold('gZ', tag, gZ, comp[1], ref[1])
    _hold('galpha', tag, galpha, comp[2], ref[2])
    # gv_out = gv u: exactly gv where fp64 is above the clamp by the margin 1e-4 gamma^2 of test_hip_softmax_sites, exactly 0 below
    g2 = math.exp(2.0 * pr['theta'][-1].item())
    live, dead = raw.detach() > 1e-4 * g2, raw.detach() < -1e-4 * g2
    assert torch.equal(gv_out[live], gv[live]) and bool((gv_out[dead] == 0).all()) and bool((gv_out[:, off] == 0).all())
    print(f'{tag}: {int(dead.sum())} of {dead.numel()} variances clamp in fp64 with the margin')
    if case == CLAMP_CASE:
        assert 0 < int((dead & (gv != 0)).sum()) and 0 < int((live & (gv != 0)).sum())
    # gQ from the same gv_out holds the rule too
    gQ = -ops.gram_moments(_dev(pr['theta']), _dev(pr['Z']), _dev(pr['X']), _dev(gv_out), _dev(gv_out), nu2)[0].cpu()
    _hold('gQ', tag, gQ, comp[3], ref[3])
    X2 = pr['X'].clone()
    if int(off.sum()):
        X2[off] = float('nan')
    for u, v, t in zip(fused, _transport(pr, gm, gv, nu2, X=X2), _transport(pr, gm, gv, nu2)):
        assert torch.equal(u, v) and torch.equal(u, t)
    print(f'{tag} composed row (gtheta gZ galpha gQ): '
          + '   '.join(f'{(c.double() - r).abs().max().item():.1e}' for c, r in zip(comp, ref)))


# -- softmax_site_bound_diff --------------------------------------------------------------------------------------------------------
# (C, Mt, N, D, F): the smallest problem; two panels, two chunks, the slab form, C in registers; C in LDS at the limit Mt = 256
BOUND_CASES = [(3, 1, 1, 1, 1), (3, 65, 513, 33, 3), (17, 256, 65, 2, 2)]
GOUT = 1.5


def _bound_problem(C, Mt, N, D, seed):
    """test_hip_sites._site_problem's recipe for C outputs, with class labels and weights with exact zeros."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, generator=g)
    Z = torch.randn(C, Mt, D, generator=g)
    theta = torch.cat([math.log(0.8 * math.sqrt(D)) + 0.1 * torch.randn(D, generator=g), torch.tensor([math.log(0.9)])])
    alpha = 0.3 * torch.randn(C, Mt, generator=g) / math.sqrt(Mt)
    R = torch.randn(C, Mt, Mt, generator=g)
    Q = (10.0 / Mt ** 2) * (R @ R.mT)
    y = torch.randint(0, C, (N,), generator=g)
    w = torch.rand(N, generator=g) + 0.25
    w[torch.randperm(N, generator=g)[:N // 3]] = 0.0
    return dict(theta=theta, Z=Z, X=X, alpha=alpha, Q=0.5 * (Q + Q.mT), y=y, w=w)


@pytest.mark.parametrize('case', BOUND_CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_softmax_site_bound_diff_against_fp64(case):
    from vargp_amd import ops, sites
    C, Mt, N, D, F = case
    pr = _bound_problem(C, Mt, N, D, seed=900 + C + Mt + N)
    names = ('theta', 'Z', 'alpha', 'Q')
    eps = ops.softmax_site_noise(NOISE_SEED, F, C, N, device=DEV)
    leaves = [pr[k].double().requires_grad_(True) for k in names]
    rval = ref_softmax_data_term(leaves[0], leaves[1], pr['X'], leaves[2], leaves[3], pr['y'], pr['w'], eps.cpu(), 0)
    ref = torch.autograd.grad(GOUT * rval.sum(), leaves)

    def device(fn):
        dl = [_dev(pr[k]).requires_grad_(True) for k in names]
        val = fn(dl[0], dl[1], _dev(pr['X']), dl[2], dl[3], _dev(pr['y']), _dev(pr['w']), F, NOISE_SEED)
        grads = torch.autograd.grad(GOUT * val.sum(), dl)
        torch.cuda.synchronize()
        return val.detach().cpu(), [t.cpu() for t in grads]

    cval, comp = device(sites.composed_softmax_site_bound)
    fval, fused = device(ops.softmax_site_bound_diff)
    tag = str(case)
    row = []
    for name, f, c, r in zip(('gtheta', 'gZ', 'galpha', 'gQ'), fused, comp, ref):
        assert bool(torch.isfinite(f).all()), name
        _hold(name, tag, f, c, r)
        row.append(f'{(c.double() - r).abs().max().item():.1e}')
    _hold('value', tag, fval, cval, rval.detach())
    print(f'{tag} composed row (gtheta gZ galpha gQ value): ' + '   '.join(row) + f'   {(cval - rval.detach()).abs().max().item():.1e}')
    assert torch.equal(fused[3], fused[3].mT)
    args = [_dev(pr[k]) for k in ('theta', 'Z', 'X', 'alpha', 'Q')]
    sums = ops.softmax_sites(*ops.site_marginals(*args), _dev(pr['y']), _dev(pr['w']), F, NOISE_SEED)[2]
    assert tuple(fval.shape) == (1,) and torch.equal(fval, sums[:1].cpu())
    # an explicit noise tensor gives the same value and gradients, bitwise
    dl = [_dev(pr[k]).requires_grad_(True) for k in names]
    val = ops.softmax_site_bound_diff(dl[0], dl[1], _dev(pr['X']), dl[2], dl[3], _dev(pr['y']), _dev(pr['w']), F, eps=eps)
    assert torch.equal(val.detach().cpu(), fval)
    for u, v in zip(torch.autograd.grad(GOUT * val.sum(), dl), fused):
        assert torch.equal(u.cpu(), v)


# -- the model ----------------------------------------------------------------------------------------------------------------------
def _model_grads(gp, x, y, route, q=None):
    bound = gp.softmax_site_bound(x.to(DEV), y.to(DEV), route=route, n_f=EM_F, seed=NOISE_SEED, q=q)
    grads = torch.autograd.grad(bound.sum(), [gp.z, gp.kernel.log_mean])
    torch.cuda.synchronize()
    return bound.detach().cpu(), [g.cpu() for g in grads]


def _fitted_prev():
    gp0, x0, y0 = em_inputs(seed=42)
    gp0 = gp0.to(DEV)
    gp0.fit_q_softmax_(x0.to(DEV), y0.to(DEV), n_iters=3, start='prior', n_f=EM_F, seed=NOISE_SEED)
    return [dict(z=gp0.z.detach().clone(), u_mean=gp0.u_mean.detach().clone(), u_tril_vec=gp0.u_tril_vec.detach().clone())]


@pytest.mark.parametrize('which', ['first', 'prev', 'matern'])
def test_model_softmax_site_bound(which):
    """M = 10, D = 2, N = 300, C = 3: the value is fit_q_softmax_(n_iters=0).bound[0] bit for bit, and torch.autograd.grad for z and
    log_mean holds the 4 x rule against the restatement (on the device's noise) for a first task, with one previous task, and
    for Matern 3/2; 'composed' forced at the same shape is the yardstick."""
    from vargp_amd import ops, sites
    prev = _fitted_prev() if which == 'prev' else []
    gp, x, y = em_inputs(kernel='matern' if which == 'matern' else 'rbf', prev=prev, turn=0.5 if prev else 0.0)
    nu2 = 3 if which == 'matern' else 0
    gp = gp.to(DEV)
    xd, yd = x.to(DEV), y.to(DEV)
    gp.fit_q_softmax_(xd, yd, n_iters=2, start='prior', n_f=EM_F, seed=NOISE_SEED)          # a q(u) away from the default start
    fit0 = gp.fit_q_softmax_(xd, yd, n_iters=0, n_f=EM_F, seed=NOISE_SEED)
    fused_val, fused = _model_grads(gp, x, y, None)
    comp_val, comp = _model_grads(gp, x, y, 'composed')
    print(f'{which}: bound {fused_val.tolist()} fit_q_softmax_(0) {fit0.bound[0].tolist()}')
    assert tuple(fused_val.shape) == (1,) and fused_val.dtype == F64 and torch.equal(fused_val, fit0.bound[0])
    a_t, H_t = (t.cpu().double() for t in sites.whitened_q(gp))
    rprev = [dict(u_mean=p['u_mean'].cpu().double(), u_tril=ref_vec2tril(p['u_tril_vec'].cpu(), EM_M).double()) for p in prev]
    z_lt = torch.cat([p['z'].cpu() for p in prev], -2).double() if prev else torch.zeros(EM_C, 0, EM_D, dtype=F64)
    leaves = [gp.z.detach().cpu().double().requires_grad_(True), gp.kernel.log_mean.detach().cpu().double().requires_grad_(True)]
    eps = ops.softmax_site_noise(NOISE_SEED, EM_F, EM_C, EM_N, device=DEV).cpu()
    val = ref_softmax_site_bound(leaves[1], z_lt, leaves[0], rprev, x, y, None, nu2, a_t, H_t, eps)
    ref = torch.autograd.grad(val.sum(), leaves)
    for name, f, c, r in zip(('z', 'log_mean'), fused, comp, ref):
        _hold(name, which, f, c, r)
    _hold('bound', which, fused_val, comp_val, val.detach())


def test_above_the_lds_limit_takes_the_composed_route():
    """Mt = 260 over two tasks: the default route is the composed one, its gradients are finite, and 'fused' is refused."""
    from vargp_amd import ops, sites
    assert sites.pick_route(None, 260, 'softmax_site_bound') == 'composed' and 260 > ops.SITE_MAX_MT
    gp0, _, _ = em_inputs(seed=44, M=130)
    prev = [dict(z=gp0.z.detach().clone().to(DEV), u_mean=0.1 * gp0.u_mean.detach().clone().to(DEV),
                 u_tril_vec=gp0.u_tril_vec.detach().clone().to(DEV))]
    gp, x, y = em_inputs(seed=45, M=130, prev=prev, turn=0.5)
    gp = gp.to(DEV)
    with pytest.raises(ValueError, match='256'):
        gp.softmax_site_bound(x.to(DEV), y.to(DEV), route='fused')
    val, grads = _model_grads(gp, x, y, None)
    assert bool(torch.isfinite(val).all()) and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in grads)


def test_fit_softmax_sites():
    """Two rounds of five Yogi steps from the prior on the host file's blobs: the trace never falls, the first round completes (the
    restatement alone gains 6e-2 |bound| there, tests/test_softmax_site_bound_host.py), z and log_mean have moved, and predict
    accepts the result."""
    gp, x, y = em_inputs()
    gp = gp.to(DEV)
    z0, th0 = gp.z.detach().clone(), gp.kernel.log_mean.detach().clone()
    fit = gp.fit_softmax_sites_(x.to(DEV), y.to(DEV), n_rounds=2, m_steps=5, start='prior', n_f=EM_F, seed=NOISE_SEED)
    tr = fit.bound
    print(f'EM trace {tr.view(-1).tolist()} rounds {fit.n_rounds} newton {fit.n_newton} stopped {fit.stopped}')
    assert tr.dtype == F64 and tuple(tr.shape) == (fit.n_rounds + 1, 1) and bool(torch.isfinite(tr).all())
    assert bool((tr[1:] >= tr[:-1]).all()) and fit.stopped in ('rounds', 'm_step') and fit.n_rounds >= 1
    assert not torch.equal(gp.z.detach(), z0) and not torch.equal(gp.kernel.log_mean.detach(), th0)
    assert gp.z.grad is None and gp.kernel.log_mean.grad is None
    with torch.no_grad():
        probs = gp.predict(x.to(DEV)).cpu()
    assert tuple(probs.shape) == (EM_N, EM_C) and bool(torch.isfinite(probs).all())
    assert (probs.argmax(-1) == y).double().mean().item() >= 0.95


def test_create_clf_q_init_em_softmax():
    from test_softmax_sites_host import blobs
    from vargp_amd.vargp import VARGP
    x, y = blobs(EM_C, EM_N, EM_D, 51)
    torch.manual_seed(5)
    gp = VARGP.create_clf(_Data(x, y), M=10, n_f=10, n_var_samples=1, map_est_hypers=True, q_init='em_softmax', em_rounds=1,
                          em_steps=3)
    assert gp.z.device.type == 'cpu'
    gp = gp.to(DEV)
    with torch.no_grad():
        probs = gp.predict(x.to(DEV)).cpu()
    assert tuple(probs.shape) == (EM_N, EM_C) and bool(torch.isfinite(probs).all())
