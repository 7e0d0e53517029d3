"""GPU: VAR-GP regression -- GaussianLikelihood (reference var_gp/likelihoods.py:66-110) on the closed-form kernels of
csrc/gauss_lik.hip and the native ELBO programs' ext_lik route:
  * the op against fp64 torch (torch.distributions.Normal + autograd) at the edges of its shape range, bitwise reproducible;
  * VARGP.loss / backward / forward / predict against golden vectors of the reference (tests/golden/make_golden_gauss.py) on
    every route: composed per-op, the program node, the block program as first task, ElboTrainer eager and captured;
  * the same against the fp64 oracle's moments at random shapes; tiled predict; retained graphs; VARGPRetrain;
  * the trainer modes that cannot take a Gaussian model refuse it; a two-task regression run learns and remembers."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import GOLDEN, PARAM_KEYS, rel_l2, to_dev, RTOL_SCALAR, REL_L2_GRAD, ATOL_PRED, RTOL_PRED

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRAD6 = ['z', 'u_mean', 'u_tril_vec', 'log_mean', 'log_logvar', 'obs_log_var']


# -- the fixtures' closed-form inputs (restated from tests/golden/make_golden_gauss.py) --------------------------------------
def targets(x, C, seed, bcast=False):
    D = x.shape[1]
    w = orc.hash_normal((C, D), seed + 201) * (2.0 / np.sqrt(max(D * 0.25, 1.0)))
    f = torch.sin(x.double() @ w.mT + torch.arange(C, dtype=torch.float64)).mT
    y = f + 0.1 * orc.hash_normal(tuple(f.shape), seed + 203)
    return (y[0] if bcast else y).float()


def load_gauss(name):
    """-> (g, params, prev, x, y, noise, obs_log_var); prev entries carry every key of the task-0 state_dict() when the
    fixture was made from one."""
    g = np.load(os.path.join(GOLDEN, f'{name}.npz'))
    S, _, C, M, D, B, n_prev, seed = [int(v) for v in g['meta']]
    olv = torch.from_numpy(g['p_obs_log_var'])
    if 'x' in g.files:
        params = {k: torch.from_numpy(g[f'p_{k}']) for k in PARAM_KEYS}
        prev = [{k: torch.from_numpy(g[f'prev{i}_{k}']) for k in ['z', 'u_mean', 'u_tril_vec']} for i in range(n_prev)]
        sd = {k[len('prev0sd_'):]: torch.from_numpy(g[k]) for k in g.files if k.startswith('prev0sd_')}
        if sd:
            prev[0].update(sd)
        noise = {k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('n_')}
        x, y = torch.from_numpy(g['x']), torch.from_numpy(g['y'])
    else:
        params, prev, x, _, noise = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=seed, kind=str(g['kind']))
        noise = {k: v for k, v in noise.items() if k != 'eps_f'}
        y = targets(x, C, seed, bool(int(g['bcast'])))
    return g, params, prev, x, y, noise, olv


def build(params, prev, S, olv, ep_var_mean=True):
    from vargp_amd.kernels import RBFKernel
    from vargp_amd.likelihoods import GaussianLikelihood
    from vargp_amd.vargp import VARGP
    D, C = params['z'].shape[-1], params['z'].shape[0]
    kern = RBFKernel(D, prior_log_mean=params['prior_log_mean'], prior_log_logvar=params['prior_log_logvar'])
    lik = GaussianLikelihood(C)
    gp = VARGP(params['z'], kern, lik, n_var_samples=S, ep_var_mean=ep_var_mean,
               prev_params=[{k: v.clone() for k, v in p.items()} for p in prev])
    with torch.no_grad():
        gp.kernel.log_mean.copy_(params['log_mean'])
        gp.kernel.log_logvar.copy_(params['log_logvar'])
        gp.u_mean.copy_(params['u_mean'])
        gp.u_tril_vec.copy_(params['u_tril_vec'])
        lik.obs_log_var.copy_(olv)
    return gp.to(DEV)


def grads6(gp):
    return dict(z=gp.z.grad, u_mean=gp.u_mean.grad, u_tril_vec=gp.u_tril_vec.grad, log_mean=gp.kernel.log_mean.grad,
                log_logvar=gp.kernel.log_logvar.grad, obs_log_var=gp.likelihood.obs_log_var.grad)


# -- op level: against fp64 torch ---------------------------------------------------------------------------------------------
def _op_inputs(S, C, B, bcast, seed):
    gen = torch.Generator().manual_seed(seed)
    mu = torch.randn(S, C, B, generator=gen)
    var = 0.05 + torch.rand(S, C, B, generator=gen)
    y = torch.randn(B if bcast else C * B, generator=gen).reshape((B,) if bcast else (C, B))
    olv = -3.0 + 2.5 * torch.rand(C, generator=gen)
    return mu, var, y, olv


def _fp64(mu, var, y, olv):
    mu, var, olv = (t.double().requires_grad_(True) for t in (mu, var, olv))
    yy = y.double() if y.dim() == 1 else y.double().unsqueeze(0)          # (B,) broadcasts over the outputs
    v = var + olv.exp().view(1, -1, 1)
    terms = -torch.distributions.Normal(mu, v.sqrt()).log_prob(yy.expand_as(mu))
    nll = terms.mean(0).mean(0).sum(0)
    g = torch.autograd.grad(2.5 * nll, [mu, var, olv])
    return nll.item(), terms.abs().sum().item() / (mu.shape[0] * mu.shape[1]), g


@pytest.mark.parametrize('S', [1, 3, 64])
@pytest.mark.parametrize('C', [1, 3, 10, 37])
@pytest.mark.parametrize('B', [1, 63, 512])
@pytest.mark.parametrize('bcast', [False, True])
def test_gauss_op_vs_fp64(S, C, B, bcast):
    from vargp_amd import ops
    mu, var, y, olv = _op_inputs(S, C, B, bcast, seed=S * 1000 + C * 10 + B + bcast)
    ref, scale, (g_mu, g_var, g_olv) = _fp64(mu, var, y, olv)
    outs = []
    for _ in range(2):
        md, vd, od = (t.to(DEV).requires_grad_(True) for t in (mu, var, olv))
        nll = ops.gauss_nll(md, vd, y.to(DEV), od)
        (2.5 * nll).backward()
        outs.append((nll.detach().cpu(), md.grad.cpu(), vd.grad.cpu(), od.grad.cpu()))
    nll, gm, gv, go = outs[0]
    assert abs(nll.item() - ref) <= 1e-5 * scale, (nll.item(), ref, scale)
    assert rel_l2(gm, g_mu) < 1e-5
    assert rel_l2(gv, g_var) < 1e-5
    assert rel_l2(go, g_olv) < 1e-5
    for a, b in zip(outs[0], outs[1]):           # no atomics: bitwise reproducible
        assert torch.equal(a, b)


def test_gauss_bwd_writes_the_forward_value():
    """The trainer's single launch (bwd with nll != NULL) leaves exactly the forward's value."""
    from vargp_amd import ops
    mu, var, y, olv = (t.to(DEV) for t in _op_inputs(3, 10, 512, False, seed=7))
    tgt = ops.gauss_target(y, 10, 512)
    a, b = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
    ops.lik_nll_fwd('gauss', mu, var, tgt, (olv,), a)
    seed = torch.tensor([3.0], device=DEV)
    gmu, gvar, go = torch.empty_like(mu), torch.empty_like(var), torch.empty_like(olv)
    ops.lik_nll_bwd('gauss', mu, var, tgt, (olv,), seed, gmu, gvar, go, nll=b)
    assert torch.equal(a, b)


# -- model level: against the reference's goldens, per route --------------------------------------------------------------------
def _loss_step(gp, g, x, y, nz):
    from vargp_amd import noise
    xd, yd = x.to(DEV), y.to(DEV)
    with noise.inject(**to_dev(nz, DEV)):
        kl_h, kl_u, nll = gp.loss(xd, yd)
        total = float(g['beta']) * kl_h + kl_u + (float(g['n_total']) / x.shape[0]) * nll
        total.backward()
        with torch.no_grad():
            pmu, pvar = gp(xd)
            pred = gp.predict(xd)
    sc = dict(kl_hypers=kl_h.item(), kl_u=kl_u.item(), nll=nll.item(), total=total.item())
    return sc, grads6(gp), pmu.cpu(), pvar.cpu(), pred.cpu()


def _check(name, g, sc, grads, pmu, pvar, pred, x):
    for k in ['kl_hypers', 'kl_u', 'nll', 'total']:
        np.testing.assert_allclose(sc[k], float(g[k]), rtol=RTOL_SCALAR, err_msg=f'{name}: {k}')
    S, C = int(g['meta'][0]), int(g['meta'][2])
    assert pred.shape == (S, C, x.shape[0])
    if 'x' in g.files:
        for k in GRAD6:
            assert rel_l2(grads[k].cpu(), g[f'grad_{k}']) < REL_L2_GRAD, (name, k)
        np.testing.assert_allclose(pmu.numpy(), g['pred_mu'], rtol=RTOL_PRED, atol=ATOL_PRED)
        np.testing.assert_allclose(pvar.numpy(), g['pred_var'], rtol=RTOL_PRED, atol=ATOL_PRED)
        np.testing.assert_allclose(pred.numpy(), g['pred_mu'], rtol=RTOL_PRED, atol=ATOL_PRED)
    else:
        for k in GRAD6:
            np.testing.assert_allclose(grads[k].double().norm().item(), float(g[f'gradnorm_{k}']), rtol=1e-3, err_msg=k)
        for k in ('log_mean', 'obs_log_var', 'u_mean'):
            assert rel_l2(grads[k].cpu(), g[f'grad_{k}']) < REL_L2_GRAD, k
        assert rel_l2(grads['z'][:, :4, :].cpu(), g['grad_z_head']) < REL_L2_GRAD
        np.testing.assert_allclose(pmu[..., :64].numpy(), g['pred_mu'], rtol=RTOL_PRED, atol=ATOL_PRED)
        np.testing.assert_allclose(pvar[..., :64].numpy(), g['pred_var'], rtol=RTOL_PRED, atol=ATOL_PRED)
        np.testing.assert_allclose(pred[..., :64].numpy(), g['pred_mu'], rtol=RTOL_PRED, atol=ATOL_PRED)


CASES = ['gauss_t0', 'gauss_t0_bcast', 'gauss_t1', 'gauss_t1_nomean', 'gauss_c20_t0', 'gauss_m112_t0', 'gauss_full_t0']


# (VARGP_T0_AS_TN concerns first-task models only: later tasks always take the block program)
ROUTES = [(n, r) for n in CASES for r in ('composed', 'program', 't0_as_tn') if r != 't0_as_tn' or '_t1' not in n]


@pytest.mark.parametrize('name,route', ROUTES)
def test_loss_grads_predict_vs_reference_golden(name, route, monkeypatch):
    g, params, prev, x, y, nz, olv = load_gauss(name)
    first = not prev
    if route == 't0_as_tn':
        monkeypatch.setenv('VARGP_T0_AS_TN', '1')
    gp = build(params, prev, int(g['meta'][0]), olv, bool(int(g['ep_var_mean'])))
    if route == 'composed':
        gp.fused_first_task = gp.fused_tasks = False
    out = _loss_step(gp, g, x, y, nz)
    # the route taken: no program for the composed route; the first-task program or the block program otherwise
    on_t0, on_tn = bool(gp._t0_progs), bool(gp._tn_progs)
    if route == 'composed':
        assert not on_t0 and not on_tn
    elif route == 't0_as_tn' or not first or int(g['meta'][3]) > 104:
        assert on_tn and not on_t0
    else:
        assert on_t0 and not on_tn
    _check(f'{name}/{route}', g, *out, x)


def test_prev_params_from_a_task0_state_dict():
    """gauss_t1's earlier task is a task-0 model's whole state_dict(), likelihood.obs_log_var included."""
    g, params, prev, x, y, nz, olv = load_gauss('gauss_t1')
    assert 'likelihood.obs_log_var' in prev[0] and 'kernel.log_mean' in prev[0]
    gp = build(params, prev, 3, olv)
    assert set(gp.prev_params[0]) <= {'z', 'u_mean', 'u_tril_vec', 'u_tril'}


@pytest.mark.parametrize('name', ['gauss_t0', 'gauss_t1', 'gauss_t1_nomean', 'gauss_m112_t0', 'gauss_full_t0'])
def test_trainer_eager_step_vs_reference_golden(name):
    """ElboTrainer.step of a Gaussian model: ext_lik program forward, one Gaussian launch, program backward; the gradients it
    leaves in .grad (after the optimiser's launch, which finishes the hyper-parameter gradients) are the reference's."""
    from vargp_amd import noise
    from vargp_amd.train import ElboTrainer
    g, params, prev, x, y, nz, olv = load_gauss(name)
    gp = build(params, prev, int(g['meta'][0]), olv, bool(int(g['ep_var_mean'])))
    tr = ElboTrainer(gp, lr=1e-3, beta=float(g['beta']), n_total=float(g['n_total']))
    assert tr._t0 and not tr.native_noise
    with noise.inject(**to_dev(nz, DEV)):
        out = tr.step(x.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    for k, v in zip(['kl_hypers', 'kl_u', 'nll'], out):
        np.testing.assert_allclose(v.item(), float(g[k]), rtol=RTOL_SCALAR, err_msg=k)
    grads = grads6(gp)
    if 'x' in g.files:
        for k in GRAD6:
            assert rel_l2(grads[k].cpu(), g[f'grad_{k}']) < REL_L2_GRAD, k
    else:
        for k in GRAD6:
            np.testing.assert_allclose(grads[k].double().norm().item(), float(g[f'gradnorm_{k}']), rtol=1e-3, err_msg=k)
        assert rel_l2(grads['obs_log_var'].cpu(), g['grad_obs_log_var']) < REL_L2_GRAD


@pytest.mark.parametrize('name', ['gauss_t0', 'gauss_t1'])
def test_trainer_graph_step_equals_eager_step(name):
    from vargp_amd import noise, ops
    from vargp_amd.train import ElboTrainer
    g, params, prev, x, y, nz, olv = load_gauss(name)
    xd, yd = x.to(DEV), y.to(DEV)
    ops.set_cholesky_error_mode('defer')
    ops.reset_linalg_errors()
    try:
        results = []
        for mode in ('eager', 'graph'):
            gp = build(params, prev, 3, olv)
            tr = ElboTrainer(gp, lr=1e-3, beta=float(g['beta']), n_total=float(g['n_total']))
            with noise.inject(**to_dev(nz, DEV)):
                if mode == 'graph':
                    tr.capture(xd, yd, warmup=2)
                    for _ in range(3):
                        out = tr.step_graph()
                else:
                    for _ in range(3):
                        out = tr.step(xd, yd)
            torch.cuda.synchronize()
            results.append(({k: v.detach().cpu().clone() for k, v in gp.state_dict().items()}, [o.item() for o in out]))
        (sd_e, out_e), (sd_g, out_g) = results
        np.testing.assert_allclose(out_g, out_e, rtol=1e-5)
        for k in sd_e:
            assert rel_l2(sd_g[k], sd_e[k]) < 1e-5, k
        assert 'likelihood.obs_log_var' in sd_e
        assert ops.linalg_error_count() == 0
    finally:
        ops.set_cholesky_error_mode('raise')


# -- fp64 oracle at random shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(2, 5, 24, 16, 48, 0, False), (3, 3, 12, 4, 40, 1, True), (1, 7, 20, 36, 70, 1, False),
                                   (2, 4, 16, 8, 96, 2, True)])
def test_program_route_vs_fp64_oracle(shape):
    from vargp_amd import noise
    S, C, M, D, B, n_prev, bcast = shape
    seed = 17 * S + 5 * C + M + D + B + n_prev
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=seed, kind='gauss')
    nz = {k: v for k, v in nz.items() if k != 'eps_f'}
    y = targets(x, C, seed, bcast)
    olv = torch.linspace(-2.0, -1.0, C)
    beta, n_total = 2.0, 10.0 * B
    names = ['z', 'u_mean', 'u_tril_vec', 'log_mean', 'log_logvar']
    leaf = {k: v.double() for k, v in params.items()}
    for k in names:
        leaf[k] = leaf[k].detach().clone().requires_grad_(True)
    lo = olv.double().requires_grad_(True)
    d = lambda o: {k: v.double() for k, v in o.items()}
    pmu, pvar, (mu_q, Lq, mu_p, Lp) = orc.forward(leaf, [d(p) for p in prev], x.double(), d(nz), want_kl=True)
    kl_u = orc.mvn_kl(mu_q, Lq, mu_p, Lp).sum(-1).mean(0).mean(0)
    kl_h = orc.kl_hypers(leaf['log_mean'], leaf['log_logvar'], leaf['prior_log_mean'], leaf['prior_log_logvar'])
    yy = y.double() if bcast else y.double().unsqueeze(0)
    nll = -torch.distributions.Normal(pmu, (pvar + lo.exp().view(1, -1, 1)).sqrt()).log_prob(yy).mean(0).mean(0).sum(0)
    total = beta * kl_h + kl_u + (n_total / B) * nll
    og = dict(zip(names + ['obs_log_var'], torch.autograd.grad(total, [leaf[k] for k in names] + [lo])))
    gp = build(params, prev, S, olv)
    xd, yd = x.to(DEV), y.to(DEV)
    with noise.inject(**to_dev(nz, DEV)):
        kh, ku, nl = gp.loss(xd, yd)
        (beta * kh + ku + (n_total / B) * nl).backward()
    assert gp._t0_progs or gp._tn_progs
    for a, b, k in [(kh, kl_h, 'kl_hypers'), (ku, kl_u, 'kl_u'), (nl, nll, 'nll')]:
        np.testing.assert_allclose(a.item(), b.item(), rtol=RTOL_SCALAR, err_msg=k)
    grads = grads6(gp)
    for k in GRAD6:
        assert rel_l2(grads[k].cpu(), og[k]) < REL_L2_GRAD, k


# -- predict, retained graph, VARGPRetrain --------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_prev,D', [(0, 8), (1, 40)])
def test_predict_shape_and_tiled_sweep(n_prev, D):
    """(S, C, B) means; a tiled sweep (per-op for first-task models, the block program's tile calls for D > 32 with earlier
    tasks) equals the single call, blocks joined along B."""
    from vargp_amd import noise
    S, C, M, B = 2, 3, 12, 100
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=41 + n_prev, kind='gauss')
    gp = build(params, prev, S, torch.full((C,), -2.0))
    xd = x.to(DEV)
    with noise.inject(eps_theta=nz['eps_theta'].to(DEV)), torch.no_grad():
        one = gp.predict(xd)
        tiled = gp.predict(xd, tile=32)
        mu, _ = gp(xd)
    assert one.shape == (S, C, B) and tiled.shape == (S, C, B)
    np.testing.assert_allclose(one.cpu().numpy(), mu.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(tiled.cpu().numpy(), one.cpu().numpy(), rtol=RTOL_PRED, atol=ATOL_PRED)


@pytest.mark.parametrize('name', ['gauss_t0', 'gauss_t1', 'gauss_m112_t0'])
def test_retained_graph_second_backward_doubles_the_gradient(name):
    from vargp_amd import noise
    g, params, prev, x, y, nz, olv = load_gauss(name)
    res = []
    for twice in (False, True):
        gp = build(params, prev, int(g['meta'][0]), olv)
        with noise.inject(**to_dev(nz, DEV)):
            kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
        loss = float(g['beta']) * kl_h + kl_u + 3.0 * nll
        if twice:
            loss.backward(retain_graph=True)
        loss.backward()
        res.append({k: v.detach().cpu().clone() for k, v in grads6(gp).items()})
    for k in GRAD6:
        assert rel_l2(res[1][k], 2 * res[0][k]) < 1e-5, k


def test_retrain_with_gaussian_likelihood_vs_reference_golden():
    from vargp_amd import noise
    from vargp_amd.kernels import RBFKernel
    from vargp_amd.likelihoods import GaussianLikelihood
    from vargp_amd.vargp_retrain import VARGPRetrain
    g = np.load(os.path.join(GOLDEN, 'retrain_gauss_wtoy_t1.npz'))
    S, _, C, M, D, B, n_prev, _ = [int(v) for v in g['meta']]
    params = {k: torch.from_numpy(g[f'p_{k}']) for k in PARAM_KEYS}
    prev = [{k: torch.from_numpy(g[f'prev{i}_{k}']) for k in ['z', 'u_mean', 'u_tril_vec']} for i in range(n_prev)]
    nz = {k[2:]: torch.from_numpy(g[k]).to(DEV) for k in g.files if k.startswith('n_')}
    x, y = torch.from_numpy(g['x']).to(DEV), torch.from_numpy(g['y']).to(DEV)
    kern = RBFKernel(D, prior_log_mean=params['prior_log_mean'], prior_log_logvar=params['prior_log_logvar'])
    gp = VARGPRetrain(params['z'], kern, GaussianLikelihood(C), n_var_samples=S,
                      prev_params=[{k: v.clone().to(DEV) for k, v in p.items()} for p in prev])
    with torch.no_grad():
        gp.kernel.log_mean.copy_(params['log_mean'])
        gp.kernel.log_logvar.copy_(params['log_logvar'])
        gp.u_mean.copy_(params['u_mean'])
        gp.u_tril_vec.copy_(params['u_tril_vec'])
        gp.likelihood.obs_log_var.copy_(torch.from_numpy(g['p_obs_log_var']))
    gp = gp.to(DEV)
    with noise.inject(**nz):
        kl_h, kl_u, nll = gp.loss(x, y)
        total = float(g['beta']) * kl_h + kl_u + (float(g['n_total']) / B) * nll
        total.backward()
        with torch.no_grad():
            pred = gp.predict(x)
    for k, v in [('kl_hypers', kl_h), ('kl_u', kl_u), ('nll', nll), ('total', total)]:
        np.testing.assert_allclose(v.item(), float(g[k]), rtol=RTOL_SCALAR, err_msg=k)
    for k, v in grads6(gp).items():
        assert rel_l2(v.cpu(), g[f'grad_{k}']) < REL_L2_GRAD, k
    for i, pd in enumerate(gp.retrain_params):
        for k in ('z', 'u_mean', 'u_tril_vec'):
            assert rel_l2(pd[k].grad.cpu(), g[f'grad_retrain{i}_{k}']) < REL_L2_GRAD, (i, k)
    assert pred.shape == (S, C, B)


# -- refusals ----------------------------------------------------------------------------------------------------------------------
def test_trainer_modes_that_assume_labels_refuse_gaussian_models(tmp_path):
    import torch.distributed as dist
    from vargp_amd import ops
    from vargp_amd.train import ElboTrainer
    g, params, prev, x, y, nz, olv = load_gauss('gauss_t0')
    xd, yd = x.to(DEV), y.to(DEV)
    gp = build(params, prev, 3, olv)
    with pytest.raises(NotImplementedError):
        gp.elbo_tiled(xd, yd, tile=50)
    ops.set_cholesky_error_mode('defer')
    try:
        tr = ElboTrainer(gp, lr=1e-3)
        tr.capture(xd, yd, warmup=1)
        with pytest.raises(NotImplementedError):
            tr.capture_unrolled(xd, yd, 2)
        with pytest.raises(NotImplementedError):
            tr.capture_epoch(xd, yd)
        with pytest.raises(NotImplementedError):
            tr.step_graph_gather(xd, yd, torch.arange(x.shape[0], device=DEV))
    finally:
        ops.set_cholesky_error_mode('raise')
    # force_exchange (the multi-rank path on one rank) and class-sharded pairs
    own = not dist.is_initialized()
    if own:
        dist.init_process_group('gloo', init_method=f'file://{tmp_path}/pg', rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError):
            ElboTrainer(build(params, prev, 3, olv), force_exchange=True)
        with pytest.raises(NotImplementedError):
            ElboTrainer(build(params, prev, 3, olv), force_exchange=True, shards=[(0, 3, 0, 4)])
    finally:
        if own:
            dist.destroy_process_group()


# -- behaviour: continual regression over two tasks ------------------------------------------------------------------------------
def _task(t, n, seed):
    gen = torch.Generator().manual_seed(seed)
    x1 = 2.5 * torch.rand(n, generator=gen) - (2.5 if t == 0 else 0.0)      # task 0: x1 in [-2.5, 0], task 1: [0, 2.5]
    x2 = 2 * torch.rand(n, generator=gen) - 1
    x = torch.stack([x1, x2], dim=-1)
    f = torch.stack([torch.sin(1.5 * x1 + c) + 0.3 * x2 for c in range(2)])            # (C = 2, n)
    return x, f + 0.05 * torch.randn(f.shape, generator=gen), f


def _rmse(gp, x, f):
    with torch.no_grad():
        mu = gp.predict(x.to(DEV)).mean(0).cpu()
    return math.sqrt(((mu - f) ** 2).mean().item())


def test_two_task_regression_learns_and_remembers():
    """300 trainer steps per task (Yogi, minibatches of 64 out of 256 points).  Bounds: the targets have RMS ~0.75; task 0 is
    fit to RMSE < 0.15 and, after task 1 has been learnt with task 0 as the previous task, still predicted to RMSE < 0.3."""
    from vargp_amd.kernels import RBFKernel
    from vargp_amd.likelihoods import GaussianLikelihood
    from vargp_amd.train import ElboTrainer
    from vargp_amd.vargp import VARGP
    torch.manual_seed(0)
    N, B, M, C, steps = 256, 64, 12, 2, 300
    data = [_task(t, N, 100 + t) for t in range(2)]
    prev, prior, models = [], (None, None), []
    for t, (x, y, f) in enumerate(data):
        z = x[torch.randperm(N)[:M]].unsqueeze(0).repeat(C, 1, 1)
        kern = RBFKernel(2, prior_log_mean=prior[0], prior_log_logvar=prior[1])
        gp = VARGP(z, kern, GaussianLikelihood(C), n_var_samples=2, prev_params=prev).to(DEV)
        tr = ElboTrainer(gp, lr=3e-2, beta=1.0, n_total=N)
        xd, yd = x.to(DEV), y.to(DEV)
        for i in range(steps):
            idx = torch.randint(0, N, (B,), device=DEV)
            out = tr.step(xd[idx], yd[:, idx])
        assert all(torch.isfinite(o).item() for o in out)
        sd = {k: v.detach().clone() for k, v in gp.state_dict().items()}
        prev = prev + [sd]
        prior = (sd['kernel.log_mean'], sd['kernel.log_logvar'])
        models.append(gp)
    r00 = _rmse(models[0], data[0][0], data[0][2])
    r10, r11 = _rmse(models[1], data[0][0], data[0][2]), _rmse(models[1], data[1][0], data[1][2])
    print(f'task-0 RMSE after task 0: {r00:.4f}; after task 1: task 0 {r10:.4f}, task 1 {r11:.4f}')
    assert r00 < 0.15
    assert r11 < 0.15
    assert r10 < 0.3
