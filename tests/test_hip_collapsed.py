"""The closed-form optimal q(u) on the device: ops.gram_moments (csrc/moments.hip), VARGP.fit_q_ (vargp_amd/collapsed.py) and
create_reg(q_init='optimal'), against the fp64 restatement of tests/test_collapsed.py.

Rule (tests/sweep_rule.py): device error against fp64 <= tolerance + 2 x the error of the fp32 restatement on one host thread.
REL_L2_GRAD (relative L2) for Phi, c, u_mean and u_tril u_tril^T; RTOL_SCALAR for the sums, the bound and kl_u; ATOL_PRED / RTOL_PRED for
predictive moments."""
import math

import pytest
import torch

from helpers import ATOL_PRED, REL_L2_GRAD, RTOL_PRED, RTOL_SCALAR, rel_l2
from test_collapsed import JITTER, _Data, ref_fit, ref_kernel, ref_moments, ref_predict, ref_vec2tril

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _one_thread(fn):
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(n)


# -- the moments --------------------------------------------------------------------------------------------------------------------
# (Mt, N, D, G, nu2, weights): Mt on both sides of one and of two 64-row tiles, N around the 64-column step and over several
# chunks, D on both sides of kRbfDirectD = 32; weights None | 'rand' | 'zeros' (random with the tail half exactly zero)
MOMENT_CASES = [
    (1, 1, 1, 1, 0, None), (15, 63, 2, 3, 1, 'rand'), (33, 64, 32, 1, 3, 'zeros'), (100, 65, 33, 3, 5, None),
    (130, 1000, 40, 1, 0, 'rand'), (15, 1000, 2, 1, 0, 'zeros'), (130, 1000, 1, 3, 3, 'rand'), (33, 1000, 33, 1, 1, 'zeros'),
    (100, 1000, 32, 1, 5, 'rand'), (1, 1000, 40, 3, 0, None), (130, 1, 2, 1, 1, None), (15, 64, 33, 3, 3, 'rand'),
    (33, 65, 1, 1, 5, 'zeros'), (100, 63, 40, 1, 0, 'zeros'), (130, 64, 32, 3, 1, None), (1, 65, 33, 1, 3, 'rand'),
    (15, 1, 40, 3, 5, 'rand'), (33, 63, 2, 1, 0, None), (100, 64, 1, 3, 1, 'zeros'), (130, 65, 2, 1, 5, 'rand'),
]


def _moment_problem(Mt, N, D, G, wmode, seed):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, generator=g)
    Z = torch.randn(G, Mt, D, generator=g)                                          # a different Z per output
    y = torch.randn(G, N, generator=g)
    theta = torch.cat([math.log(0.8 * math.sqrt(D)) + 0.1 * torch.randn(D, generator=g), torch.tensor([math.log(0.9)])])
    w = None if wmode is None else torch.rand(G, N, generator=g) + 0.25
    keep = N
    if wmode == 'zeros':
        keep = N // 2
        w[:, keep:] = 0.0
    return theta, Z, X, w, y, keep


def _hold_to_rule(got, r32, r64, tag):
    (Phi, c, sums), (P32, c32, s32), (P64, c64, s64) = got, r32, r64
    for name, a, b32, b64 in (('Phi', Phi, P32, P64), ('c', c, c32, c64)):
        for g in range(b64.shape[0]):
            e, e32 = rel_l2(a[g], b64[g]), rel_l2(b32[g], b64[g])
            print(f'{tag} {name}[{g}]: err {e:.2e} (fp32 host {e32:.2e})')
            assert e <= REL_L2_GRAD + 2.0 * e32, (tag, name, g, e, e32)
    es = ((sums.double() - s64).abs() / s64.abs().clamp_min(1e-30)).max().item()
    es32 = ((s32.double() - s64).abs() / s64.abs().clamp_min(1e-30)).max().item()
    print(f'{tag} sums: err {es:.2e} (fp32 host {es32:.2e})')
    assert es <= RTOL_SCALAR + 2.0 * es32, (tag, es, es32)


@pytest.mark.parametrize('Mt,N,D,G,nu2,wmode', MOMENT_CASES, ids=['-'.join(map(str, c)) for c in MOMENT_CASES])
def test_moments_against_fp64(Mt, N, D, G, nu2, wmode):
    from vargp_amd import ops
    theta, Z, X, w, y, keep = _moment_problem(Mt, N, D, G, wmode, seed=Mt + 7 * N + 13 * D)
    dev = lambda t: None if t is None else t.to(DEV)
    call = lambda X_, w_, y_: [t.cpu() for t in ops.gram_moments(dev(theta), dev(Z), dev(X_), dev(w_), dev(y_), nu2)]
    got = call(X, w, y)
    Phi, c, sums = got
    assert Phi.shape == (G, Mt, Mt) and c.shape == (G, Mt) and sums.shape == (G, 2)
    assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in got)
    assert torch.equal(Phi, Phi.mT)                                                 # exactly symmetric
    junk = torch.full((1 << 20,), float('nan'), device=DEV)                         # (the pooled scratch is reused: poison what follows it)
    again = call(X, w, y)
    del junk
    assert all(torch.equal(u, v) for u, v in zip(got, again))                       # two calls are bitwise equal
    r64 = ref_moments(theta, Z, X, w, y, nu2)
    r32 = _one_thread(lambda: ref_moments(theta, Z, X, w, y, nu2, dtype=torch.float32))
    tag = f'Mt{Mt} N{N} D{D} G{G} nu2={nu2} w={wmode}'
    _hold_to_rule(got, r32, r64, tag)
    if wmode == 'zeros' and keep >= 1:
        # the zero-weight points removed: the same sums.  With one chunk on both sides the kept points sit in the same columns of
        # the same steps and a zero weight adds exactly +0: bitwise equal; with other chunkings the results are held to the rule
        cut = call(X[:keep], w[:, :keep], y[:, :keep])
        if ops.gram_moments_chunks(G, Mt, N, D) == 1 and ops.gram_moments_chunks(G, Mt, keep, D) == 1:
            assert all(torch.equal(u, v) for u, v in zip(got, cut)), tag
        else:
            _hold_to_rule(cut, r32, r64, tag + ' (removed)')


def test_a_multi_chunk_case_is_covered():
    from vargp_amd import ops
    multi = [c for c in MOMENT_CASES if ops.gram_moments_chunks(c[3], c[0], c[1], c[2]) > 1]
    assert multi and any(c[2] <= 32 for c in multi) and any(c[2] > 32 for c in multi), multi
    assert ops.gram_moments_chunks(1, 15, 1000, 2) > 1


def test_padding_columns_are_masked_not_weighted():
    """N = 70 points at the head of a buffer whose next rows are NaN, in a 128-column chunk: nothing behind row N is used."""
    from vargp_amd import ops
    theta, Z, X, w, y, _ = _moment_problem(33, 70, 5, 2, 'rand', seed=5)
    Xbig = torch.full((256, 5), float('nan'))
    Xbig[:70] = X
    a = ops.gram_moments(theta.to(DEV), Z.to(DEV), X.to(DEV), w.to(DEV), y.to(DEV), 0)
    b = ops.gram_moments(theta.to(DEV), Z.to(DEV), Xbig.to(DEV)[:70], w.to(DEV), y.to(DEV), 0)
    assert all(torch.equal(u, v) and bool(torch.isfinite(u).all()) for u, v in zip(a, b))


def test_einval_raises():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    theta, Z, X, w, y = [t.to(DEV) for t in _moment_problem(5, 9, 3, 2, 'rand', seed=1)[:5]]
    for nu2 in (2, -1, 7):
        with pytest.raises(VargpHipError, match='nu2'):
            ops.gram_moments(theta, Z, X, w, y, nu2)
    with pytest.raises(VargpHipError):                                              # N = 0
        ops.gram_moments(theta, Z, X[:0], None, y[:, :0], 0)
    # (G > 65535, null pointers and a short workspace: tests/test_collapsed.py, at the C ABI with host memory)


# -- the solver ---------------------------------------------------------------------------------------------------------------------
def _task_data(N, D, C, task, scale):
    g = torch.Generator().manual_seed(100 + task)
    x = scale * torch.randn(N, D, generator=g) + 0.5 * scale * task
    t = torch.stack([torch.sin(1.5 * x[:, 0] / scale + c) + 0.3 * x[:, -1] / scale for c in range(C)], -1)
    t = t + 0.1 * torch.randn(N, C, generator=g)
    return _Data(x, t[:, 0].contiguous() if C == 1 else t)


def _chain(C, M, n_prev, kernel, D, N=200, **kw):
    """create_reg task by task (each earlier task fitted and handed over as prev_params); -> (model of the last task on the
    device BEFORE its fit, its data set)."""
    from vargp_amd.vargp import VARGP
    scale = 1.0 if D <= 8 else 0.12                                                 # (lengthscale 0.5: keep the kernel away from gamma^2 I)
    prev = None
    for task in range(n_prev + 1):
        data = _task_data(N, D, C, task, scale)
        torch.manual_seed(task)
        gp = VARGP.create_reg(data, M=M, kernel=kernel, map_est_hypers=True,
                              prev_params=None if prev is None else [dict(p) for p in prev], **kw).to(DEV)
        if task < n_prev:
            y = data.targets if C == 1 else data.targets.t()
            gp.fit_q_(data.x.to(DEV), y.to(DEV))
            sd = {k: v.detach().cpu().clone() for k, v in gp.state_dict().items()}
            prev = (prev or []) + [sd]               # (create_reg gets copies: it pops the kernel.* keys of what it is given)
    return gp, data


def _restate(gp, data, C, dtype):
    nu2 = int(round(2 * gp.kernel.nu)) if hasattr(gp.kernel, 'nu') else 0
    M = gp.M
    prev = [dict(z=p['z'].cpu(), u_mean=p['u_mean'].cpu(), u_tril=ref_vec2tril(p['u_tril_vec'].cpu().to(dtype), M)) for p in gp.prev_params]
    z_all = torch.cat([p['z'] for p in prev] + [gp.z.detach().cpu()], -2)
    y = (data.targets.unsqueeze(0) if C == 1 else data.targets.t()).contiguous()
    theta, olv = gp.kernel.log_mean.detach().cpu(), gp.likelihood.obs_log_var.detach().cpu()
    return ref_fit(theta, z_all, prev, data.x, y, None, olv, nu2, dtype=dtype), (theta, z_all, prev, nu2)


SOLVER_CASES = [(1, 5, 0, 'rbf', 3), (2, 33, 0, 'matern32', 3), (2, 5, 2, 'rbf', 40), (1, 33, 2, 'matern32', 3), (2, 33, 2, 'rbf', 3)]


@pytest.mark.parametrize('C,M,n_prev,kernel,D', SOLVER_CASES, ids=['-'.join(map(str, c)) for c in SOLVER_CASES])
def test_fit_q_against_the_restatement(C, M, n_prev, kernel, D):
    from vargp_amd import noise
    from vargp_amd.gp_utils import rev_cholesky, vec2tril
    gp, data = _chain(C, M, n_prev, kernel, D)
    x = data.x.to(DEV)
    y = (data.targets if C == 1 else data.targets.t().contiguous()).to(DEV)
    before = gp.u_mean.detach().clone()
    fit = gp.fit_q_(x, y)
    assert fit.bound.shape == (C,) and fit.bound.dtype == torch.float64 and fit.n_chunks >= 1
    assert not torch.equal(before, gp.u_mean.detach())
    f64, (theta, z_all, prev, nu2) = _restate(gp, data, C, torch.float64)
    f32, _ = _one_thread(lambda: _restate(gp, data, C, torch.float32))
    tag = f'C{C} M{M} t{n_prev} {kernel} D{D}'
    # parameters and bound
    with torch.no_grad():
        S_dev = rev_cholesky(vec2tril(gp.u_tril_vec, M)).cpu()
    S64, S32 = f64['u_tril'] @ f64['u_tril'].mT, f32['u_tril'] @ f32['u_tril'].mT
    for name, a, b32, b64 in (('u_mean', gp.u_mean.detach().cpu().squeeze(-1), f32['u_mean'], f64['u_mean']), ('S_u', S_dev, S32, S64)):
        e, e32 = rel_l2(a, b64), rel_l2(b32, b64)
        print(f'{tag} {name}: err {e:.2e} (fp32 host {e32:.2e})')
        assert e <= REL_L2_GRAD + 2.0 * e32, (tag, name, e, e32)
    eb = ((fit.bound.cpu() - f64['bound']).abs() / f64['bound'].abs()).max().item()
    eb32 = ((f32['bound'].double() - f64['bound']).abs() / f64['bound'].abs()).max().item()
    print(f'{tag} bound {fit.bound.tolist()}: err {eb:.2e} (fp32 host {eb32:.2e})')
    assert eb <= RTOL_SCALAR + 2.0 * eb32, (tag, eb, eb32)
    # a second fit leaves the parameters bitwise unchanged
    um, uv = gp.u_mean.detach().clone(), gp.u_tril_vec.detach().clone()
    fit2 = gp.fit_q_(x, y)
    assert torch.equal(um, gp.u_mean.detach()) and torch.equal(uv, gp.u_tril_vec.detach()) and torch.equal(fit.bound, fit2.bound)
    # kl_u of VARGP.loss is the KL of the whitened block
    kl_u = gp.loss(x[:64], y[..., :64])[1].detach().item()
    k64, k32 = f64['kl'].sum().item(), f32['kl'].double().sum().item()
    ek, ek32 = abs(kl_u - k64) / abs(k64), abs(k32 - k64) / abs(k64)
    print(f'{tag} kl_u {kl_u:.6g} vs {k64:.6g}: err {ek:.2e} (fp32 host {ek32:.2e})')
    assert ek <= RTOL_SCALAR + 2.0 * ek32, (tag, ek, ek32)
    # predictive moments of the fitted model
    xs = data.x[:50] + 0.1 * data.x[50:100]
    with noise.inject(eps_theta=torch.zeros(1, theta.numel(), device=DEV)):
        mu, var = gp.predict_f(xs.to(DEV))
    assert mu.shape == (1, C, 50)
    pred = lambda f, dt: ref_predict(theta, z_all, [p['u_mean'] for p in prev] + [f['u_mean'].unsqueeze(-1)],
                                     [p['u_tril'] for p in prev] + [f['u_tril']], xs, nu2, dtype=dt)
    (m64, v64), (m32, v32) = pred(f64, torch.float64), _one_thread(lambda: pred(f32, torch.float32))
    for name, a, b32, b64 in (('mu', mu[0].cpu(), m32, m64), ('var', var[0].cpu(), v32, v64)):
        e32 = (b32.double() - b64).abs().max().item()
        over = ((a.double() - b64).abs() - (ATOL_PRED + RTOL_PRED * b64.abs() + 2.0 * e32)).max().item()
        print(f'{tag} pred {name}: max err {(a.double() - b64).abs().max().item():.2e} (fp32 host {e32:.2e})')
        assert over <= 0.0, (tag, name, over)


def test_exact_gp_when_the_inducing_points_are_the_data():
    """N = M = 12: z is the training set, so the fitted mean is the exact GP posterior mean up to the jitter -- the device's gap is no
    more than the fp64 restatement's own gap plus the rule's bound."""
    from vargp_amd.vargp import VARGP
    data = _task_data(12, 2, 1, 0, 1.0)
    torch.manual_seed(0)
    gp = VARGP.create_reg(data, M=12, map_est_hypers=True).to(DEV)
    assert torch.equal(gp.z.detach().cpu()[0].sort(0)[0], data.x.sort(0)[0])
    gp.fit_q_(data.x.to(DEV), data.targets.to(DEV))
    f64, (theta, z_all, _, _) = _restate(gp, data, 1, torch.float64)
    f32, _ = _one_thread(lambda: _restate(gp, data, 1, torch.float32))
    xs = torch.randn(20, 2, generator=torch.Generator().manual_seed(1))
    mu = gp.predict_f(xs.to(DEV))[0][0, 0].cpu().double()
    m64 = ref_predict(theta, z_all, [f64['u_mean'].unsqueeze(-1)], [f64['u_tril']], xs, 0)[0][0]
    m32 = _one_thread(lambda: ref_predict(theta, z_all, [f32['u_mean'].unsqueeze(-1)], [f32['u_tril']], xs, 0, dtype=torch.float32))[0][0]
    th, x64 = theta.double(), data.x.double()
    Kxx = ref_kernel(x64, x64, th, 0) + gp.likelihood.obs_log_var.detach().cpu().double().exp() * torch.eye(12, dtype=torch.float64)
    exact = ref_kernel(xs.double(), x64, th, 0) @ torch.linalg.solve(Kxx, data.targets.double())
    gap, gap64, e32 = (mu - exact).abs(), (m64 - exact).abs().max().item(), (m32.double() - m64).abs().max().item()
    print(f'exact GP: device gap {gap.max().item():.2e}, fp64 restatement gap {gap64:.2e} (jitter {JITTER}), fp32 host err {e32:.2e}')
    assert bool((gap <= gap64 + ATOL_PRED + RTOL_PRED * exact.abs() + 2.0 * e32).all())


@pytest.mark.parametrize('n_prev', [0, 1])
def test_q_init_optimal_is_create_reg_then_fit(n_prev):
    from vargp_amd.vargp import VARGP
    gp0, data = _chain(2, 5, n_prev, 'rbf', 3)
    prev = [dict(z=p['z'].cpu(), u_mean=p['u_mean'].cpu(), u_tril_vec=p['u_tril_vec'].cpu()) for p in gp0.prev_params]
    made = []
    for q_init in ('default', 'optimal'):
        torch.manual_seed(9)
        gp = VARGP.create_reg(data, M=5, prev_params=[dict(p) for p in prev] or None, q_init=q_init)
        assert gp.z.device == data.x.device                                         # back where the default route leaves it
        made.append(gp.to(DEV))
    made[0].fit_q_(data.x.to(DEV), data.targets.t().contiguous().to(DEV))
    a, b = made[0].state_dict(), made[1].state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
