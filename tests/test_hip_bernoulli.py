"""GPU: BernoulliLikelihood (csrc/indep_lik.hip; not in the reference, so no reference goldens).  Yardstick: the fp64
restatement `rule()` below -- the 20-node Gauss-Hermite sum that DEFINES the likelihood, with torch.special.log_ndtr /
-softplus(-z) and torch.autograd -- at op level on a grid of shapes, links, target forms and input ranges, and at model level
on top of the fp64 oracle's predictive moments and KL ingredients, per route (composed, first-task program, block program,
trainer eager and captured, VARGPRetrain).  Behaviour: a two-task run against the softmax model.

Op-level bounds.  Typical inputs: the Gaussian op test's (value within 1e-5 x sum|terms| / S, rel_l2 < 1e-5 per gradient).
Wide and edge inputs: plain fp32 arithmetic itself loses digits on the variance gradient there (f_k = mu + sqrt(2 var) x_k is
rounded to ulp(mu)), so the same rule is evaluated in fp32 torch on the CPU on the same inputs and the kernel is allowed
max(1e-5, 4 x that error) per quantity -- the factor 4 for a different summation order.  The bound comes from that independent
implementation, never from the kernel."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vargp_oracle as orc
from helpers import ATOL_PROBS, REL_L2_GRAD, RTOL_SCALAR, rel_l2, to_dev

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ['z', 'u_mean', 'u_tril_vec', 'log_mean', 'log_logvar']
SEED = 2.5


# -- the fp64 yardstick ---------------------------------------------------------------------------------------------------------
def rule(mu, var, t, link):
    """ell (S, C, B) of the 20-node rule in the dtype of mu; t (C, B) or (B,) in {0, 1}."""
    x, w = np.polynomial.hermite.hermgauss(20)
    x, w = torch.tensor(x, dtype=mu.dtype), torch.tensor(w / np.sqrt(np.pi), dtype=mu.dtype)
    z = (2 * t.to(mu.dtype) - 1).unsqueeze(-1) * (mu.unsqueeze(-1) + (2 * var).sqrt().unsqueeze(-1) * x)
    lp = torch.special.log_ndtr(z) if link == 'probit' else -F.softplus(-z)
    return (lp * w).sum(-1)


def rule_nll(mu, var, t, link):
    return -rule(mu, var, t, link).mean(0).sum()


def rule_probs(mu, var, link):
    """(B, C) = mean_s P(t = 1): probit in closed form, logit by the rule."""
    if link == 'probit':
        p = torch.special.ndtr(mu / (1 + var).sqrt())
    else:
        x, w = np.polynomial.hermite.hermgauss(20)
        x, w = torch.tensor(x, dtype=mu.dtype), torch.tensor(w / np.sqrt(np.pi), dtype=mu.dtype)
        p = (torch.sigmoid(mu.unsqueeze(-1) + (2 * var).sqrt().unsqueeze(-1) * x) * w).sum(-1)
    return p.mean(0).t()


def _ref(mu, var, t, link, dtype):
    """-> (nll, sum|terms| / S, gmu, gvar) of SEED * nll in `dtype` on the CPU."""
    m, v = (a.detach().to(dtype).clone().requires_grad_(True) for a in (mu, var))      # (never the caller's tensors)
    ell = rule(m, v, t, link)
    nll = -ell.mean(0).sum()
    gm, gv = torch.autograd.grad(SEED * nll, [m, v])
    return nll.item(), ell.detach().abs().sum().item() / mu.shape[0], gm, gv


def _inputs(S, C, B, rng, seed):
    gen = torch.Generator().manual_seed(seed)
    n = torch.randn(S, C, B, generator=gen)
    u = torch.rand(S, C, B, generator=gen)
    if rng == 'typical':
        mu, var = 2 * n, 0.01 + 1.99 * u
    elif rng == 'wide':
        mu, var = 8 * n, torch.exp(math.log(1e-4) + u * (math.log(25.0) - math.log(1e-4)))
    else:
        mu, var = (30 * n).clamp(-30, 30), torch.exp(math.log(1e-6) + u * (math.log(100.0) - math.log(1e-6)))
    assert mu.dtype == torch.float32 and var.dtype == torch.float32
    labels = torch.randint(0, C, (B,), generator=gen)
    multi = (torch.rand(C, B, generator=gen) < 0.4).float()
    return mu, var, labels, multi


def _run(mu, var, y, link):
    from vargp_amd import ops
    md, vd = (a.detach().to(DEV).requires_grad_(True) for a in (mu, var))
    nll = ops.bernoulli_nll(md, vd, y.to(DEV), link)
    (SEED * nll).backward()
    return nll.detach().cpu(), md.grad.cpu(), vd.grad.cpu()


@pytest.mark.parametrize('rng', ['typical', 'wide', 'edge'])
@pytest.mark.parametrize('link', ['probit', 'logit'])
@pytest.mark.parametrize('B', [1, 63, 512])
@pytest.mark.parametrize('C', [1, 3, 10, 37])
@pytest.mark.parametrize('S', [1, 3, 64])
def test_op_vs_fp64_rule(S, C, B, link, rng):
    mu, var, labels, multi = _inputs(S, C, B, rng, seed=S * 1000 + C * 10 + B)
    onehot = (labels.unsqueeze(0) == torch.arange(C).unsqueeze(1)).float()
    forms = [('labels', labels, onehot), ('onehot', onehot, onehot), ('multi', multi, multi), ('shared', multi[0], multi[0])]
    got = {}
    for name, y, t in forms:
        ref, scale, g_mu, g_var = _ref(mu, var, t, link, torch.float64)
        if rng == 'typical':
            b_val = b_mu = b_var = 1e-5
        else:
            r32, _, m32, v32 = _ref(mu, var, t, link, torch.float32)
            b_val = max(1e-5, 4 * abs(r32 - ref) / scale)
            b_mu, b_var = max(1e-5, 4 * rel_l2(m32, g_mu)), max(1e-5, 4 * rel_l2(v32, g_var))
        a, b = _run(mu, var, y, link), _run(mu, var, y, link)
        nll, gm, gv = got[name] = a
        e_val, e_mu, e_var = abs(nll.item() - ref) / scale, rel_l2(gm, g_mu), rel_l2(gv, g_var)
        print(f'[op] S{S} C{C} B{B} {link} {rng} {name}: value {e_val:.2e} (bound {b_val:.2e}) gmu {e_mu:.2e} ({b_mu:.2e}) '
              f'gvar {e_var:.2e} ({b_var:.2e})', flush=True)
        assert all(torch.isfinite(q).all() for q in a), name
        assert e_val <= b_val, (name, nll.item(), ref, scale)
        assert e_mu < b_mu, name
        assert e_var < b_var, name
        for p, q in zip(a, b):                        # no float atomics: bitwise reproducible
            assert torch.equal(p, q), name
    for p, q in zip(got['labels'], got['onehot']):    # one-vs-rest labels == the one-hot float targets, bitwise
        assert torch.equal(p, q)


@pytest.mark.parametrize('link', ['probit', 'logit'])
@pytest.mark.parametrize('shape', [(3, 10, 512), (64, 37, 512), (1, 1, 1), (2, 5, 63)])
def test_bwd_writes_the_forward_value(shape, link):
    """The trainer's single call (bwd with nll) leaves exactly the forward's value."""
    from vargp_amd import ops
    S, C, B = shape
    mu, var, labels, multi = (a.to(DEV) for a in _inputs(S, C, B, 'wide', seed=7))
    for y in (labels, multi):
        tgt = ops.bernoulli_target(y, C, B)
        a, b = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
        ops.lik_nll_fwd('bernoulli', mu, var, tgt, (ops.BERNOULLI_LINKS[link],), a)
        gmu, gvar = torch.empty_like(mu), torch.empty_like(var)
        ops.lik_nll_bwd('bernoulli', mu, var, tgt, (ops.BERNOULLI_LINKS[link],), torch.tensor([3.0], device=DEV), gmu, gvar, nll=b)
        assert torch.equal(a, b)


def test_c_abi_argument_checks():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError, lib, ptr, stream_ptr
    mu, var = torch.zeros(2, 3, 4, device=DEV), torch.ones(2, 3, 4, device=DEV)
    t, lab = torch.zeros(3, 4, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    out, ws = torch.zeros(1, device=DEV), torch.zeros(64, device=DEV)
    call = lambda t_, l_, link, ldt=4, wsb=256: lib().vargp_bernoulli_nll_fwd(
        ptr(mu), ptr(var), ptr(t_), ldt, ptr(l_), link, ptr(out), 2, 3, 4, ptr(ws), wsb, stream_ptr())
    assert call(t, None, 0) == 0 and call(None, lab, 1) == 0
    assert call(t, lab, 0) != 0 and call(None, None, 0) != 0          # exactly one target pointer
    assert call(t, None, 2) != 0 and call(t, None, -1) != 0            # link in {0, 1}
    assert call(t, None, 0, ldt=3) != 0 and call(t, None, 0, wsb=0) != 0
    with pytest.raises(VargpHipError):
        ops.lik_nll_fwd('bernoulli', mu, var, (t, 4, lab), (0,), out)
    torch.cuda.synchronize()


def test_out_of_range_labels_match_no_output():
    from vargp_amd import ops
    mu, var, _, _ = _inputs(2, 3, 8, 'typical', seed=3)
    labels = torch.tensor([0, 1, 2, 3, -1, 99, 2, 0])
    t = (labels.unsqueeze(0) == torch.arange(3).unsqueeze(1)).float()
    a = ops.bernoulli_nll(mu.to(DEV), var.to(DEV), labels.to(DEV))
    b = ops.bernoulli_nll(mu.to(DEV), var.to(DEV), t.to(DEV))
    assert torch.equal(a, b) and torch.isfinite(a)


@pytest.mark.parametrize('link', ['probit', 'logit'])
@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 10, 512), (64, 37, 63)])
def test_predict_and_forward_vs_fp64(shape, link):
    from vargp_amd.likelihoods import BernoulliLikelihood
    S, C, B = shape
    mu, var, _, _ = _inputs(S, C, B, 'wide', seed=11)
    lik = BernoulliLikelihood(link)
    probs = lik.predict(mu.to(DEV), var.to(DEV)).cpu()
    assert probs.shape == (B, C)
    np.testing.assert_allclose(probs.numpy(), rule_probs(mu.double(), var.double(), link).numpy(), atol=ATOL_PROBS)
    if link == 'probit':       # the closed form itself
        want = torch.special.ndtr(mu.double() / (1 + var.double()).sqrt()).mean(0).t()
        np.testing.assert_allclose(probs.numpy(), want.numpy(), atol=ATOL_PROBS)
    per = lik(mu.to(DEV), var.to(DEV)).cpu()
    assert per.shape == (S, C, B)
    np.testing.assert_allclose(per.mean(0).t().numpy(), probs.numpy(), atol=1e-6)


# -- model level: the fp64 oracle's moments and KL, the fp64 rule on top --------------------------------------------------------
def _build(params, prev, S, link, kernel='rbf', ep_var_mean=True, phi=None, cls=None):
    from vargp_amd.kernels import DeepRBFKernel, MaternKernel, RBFKernel
    from vargp_amd.likelihoods import BernoulliLikelihood
    from vargp_amd.vargp import VARGP
    D = params['z'].shape[-1]
    kw = dict(prior_log_mean=params['prior_log_mean'], prior_log_logvar=params['prior_log_logvar'])
    if kernel == 'rbf':
        kern = RBFKernel(D, **kw)
    elif kernel == 'dkl':
        kern = DeepRBFKernel(D, **kw)
        kern.phi.load_state_dict(phi)
    else:
        kern = MaternKernel(D, nu=kernel, native=True, **kw)
    pp = [{k: v.clone() for k, v in p.items()} for p in prev]
    if cls is not None:
        gp = cls(params['z'], kern, BernoulliLikelihood(link), n_var_samples=S, prev_params=to_dev(pp, DEV))
    else:
        gp = VARGP(params['z'], kern, BernoulliLikelihood(link), n_var_samples=S, ep_var_mean=ep_var_mean, prev_params=pp)
    with torch.no_grad():
        gp.kernel.log_mean.copy_(params['log_mean'])
        gp.kernel.log_logvar.copy_(params['log_logvar'])
        gp.u_mean.copy_(params['u_mean'])
        gp.u_tril_vec.copy_(params['u_tril_vec'])
    return gp.to(DEV)


def _grads(gp):
    return dict(z=gp.z.grad, u_mean=gp.u_mean.grad, u_tril_vec=gp.u_tril_vec.grad, log_mean=gp.kernel.log_mean.grad,
                log_logvar=gp.kernel.log_logvar.grad)


def _targets(kind, C, B, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == 'labels':
        y = torch.randint(0, C, (B,), generator=gen)
        return y, (y.unsqueeze(0) == torch.arange(C).unsqueeze(1)).double()
    y = (torch.rand(C, B, generator=gen) < 0.4).float()
    return y, y.double()


def _oracle(params, prev, x, nz, t, link, beta, scale, ep_var_mean=True):
    """fp64: (kl_hypers, kl_u, nll) and the gradients of beta kl_hypers + kl_u + scale nll with respect to NAMES."""
    d = lambda o: {k: v.double() for k, v in o.items()}
    leaf = d(params)
    for k in NAMES:
        leaf[k] = leaf[k].detach().clone().requires_grad_(True)
    pmu, pvar, (mu_q, Lq, mu_p, Lp) = orc.forward(leaf, [d(p) for p in prev], x.double(), d(nz), want_kl=True,
                                                  ep_var_mean=ep_var_mean)
    kl_u = orc.mvn_kl(mu_q, Lq, mu_p, Lp).sum(-1).mean(0).mean(0)
    kl_h = orc.kl_hypers(leaf['log_mean'], leaf['log_logvar'], leaf['prior_log_mean'], leaf['prior_log_logvar'])
    nll = rule_nll(pmu, pvar, t, link)
    grads = torch.autograd.grad(beta * kl_h + kl_u + scale * nll, [leaf[k] for k in NAMES])
    return (kl_h, kl_u, nll), dict(zip(NAMES, grads))


# (S, C, M, D, B, n_prev), route, targets, link, kernel, ep_var_mean -> the program expected: 't0' | 'tn' | None
CASES = [
    ((2, 5, 24, 16, 48, 0), 'program', 'labels', 'probit', 'rbf', True, 't0'),
    ((2, 5, 24, 16, 48, 0), 'composed', 'multi', 'logit', 'rbf', True, None),
    ((2, 5, 24, 16, 48, 0), 't0_as_tn', 'labels', 'logit', 'rbf', True, 'tn'),
    ((3, 3, 12, 4, 40, 1), 'program', 'multi', 'probit', 'rbf', True, 'tn'),
    ((3, 3, 12, 4, 40, 1), 'composed', 'labels', 'probit', 'rbf', True, None),
    ((1, 7, 20, 36, 70, 1), 'program', 'labels', 'probit', 'rbf', True, 'tn'),
    ((2, 4, 16, 8, 96, 2), 'program', 'multi', 'logit', 'rbf', True, 'tn'),
    ((2, 3, 112, 8, 64, 0), 'program', 'labels', 'probit', 'rbf', True, 'tn'),
    ((2, 3, 12, 40, 40, 1), 'program', 'labels', 'probit', 'rbf', False, 'tn'),
    ((2, 3, 12, 8, 40, 1), 'program', 'labels', 'probit', 1.5, True, 'tn'),
    ((2, 3, 12, 8, 40, 0), 'program', 'multi', 'probit', 'dkl', True, None),
]


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c[0]) + f'-{c[1]}-{c[2]}-{c[3]}-{c[4]}-{c[5]}')
def test_loss_and_grads_vs_fp64_oracle(case, monkeypatch):
    from vargp_amd import noise
    (S, C, M, D, B, n_prev), route, kind, link, kernel, ep_var_mean, expect = case
    seed = 17 * S + 5 * C + M + D + B + n_prev
    phi = None
    if kernel == 'dkl':
        params, prev, x, _, nz, phi = orc.make_dkl_problem(S, 1, C, M, D, B, n_prev, seed)
    else:
        params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=seed, kind='gauss')
    nz = {k: v for k, v in nz.items() if k != 'eps_f'}
    if route == 't0_as_tn':
        monkeypatch.setenv('VARGP_T0_AS_TN', '1')
    if isinstance(kernel, float):
        from test_hip_matern import matern_ref
        monkeypatch.setattr(orc, 'rbf_gram', lambda theta, a, b=None, full_gram=False: matern_ref(theta, a, b, nu=kernel))
    y, t = _targets(kind, C, B, seed)
    beta, n_total = 2.0, 10.0 * B
    if phi is not None:
        with orc.deep_kernel({k: v.double() for k, v in phi.items()}):
            (kl_h, kl_u, nll), og = _oracle(params, prev, x, nz, t, link, beta, n_total / B, ep_var_mean)
    else:
        (kl_h, kl_u, nll), og = _oracle(params, prev, x, nz, t, link, beta, n_total / B, ep_var_mean)
    gp = _build(params, prev, S, link, kernel, ep_var_mean, phi)
    if route == 'composed':
        gp.fused_first_task = gp.fused_tasks = False
    with noise.inject(**to_dev(nz, DEV)):
        kh, ku, nl = gp.loss(x.to(DEV), y.to(DEV))
        (beta * kh + ku + (n_total / B) * nl).backward()
    on_t0, on_tn = bool(gp._t0_progs), bool(gp._tn_progs)
    assert (on_t0, on_tn) == (expect == 't0', expect == 'tn'), (on_t0, on_tn, expect)
    if isinstance(kernel, float):
        assert all(p.kernel_nu2 == 3 for p in gp._tn_progs.values())
    for a, b, k in [(kh, kl_h, 'kl_hypers'), (ku, kl_u, 'kl_u'), (nl, nll, 'nll')]:
        np.testing.assert_allclose(a.item(), b.item(), rtol=RTOL_SCALAR, err_msg=k)
    for k, g in _grads(gp).items():
        assert rel_l2(g.cpu(), og[k]) < REL_L2_GRAD, k


@pytest.mark.parametrize('shape', [(2, 5, 24, 16, 48, 0), (3, 3, 12, 4, 40, 1), (2, 3, 112, 8, 64, 0)])
@pytest.mark.parametrize('kind', ['labels', 'multi'])
def test_trainer_eager_step_vs_fp64_oracle(shape, kind):
    """ElboTrainer.step: ext_lik program forward, ONE Bernoulli call (value + seeded gradients), program backward."""
    from vargp_amd import noise
    from vargp_amd.train import ElboTrainer
    S, C, M, D, B, n_prev = shape
    seed = 3 + sum(shape)
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=seed, kind='gauss')
    nz = {k: v for k, v in nz.items() if k != 'eps_f'}
    y, t = _targets(kind, C, B, seed)
    beta, n_total = 2.0, 10.0 * B
    sc, og = _oracle(params, prev, x, nz, t, 'probit', beta, n_total / B)
    gp = _build(params, prev, S, 'probit')
    tr = ElboTrainer(gp, lr=1e-3, beta=beta, n_total=n_total)
    assert tr._t0 and tr.ext and not tr.native_noise
    with noise.inject(**to_dev(nz, DEV)):
        out = tr.step(x.to(DEV), y.to(DEV))
    torch.cuda.synchronize()
    for a, b, k in zip(out, sc, ['kl_hypers', 'kl_u', 'nll']):
        np.testing.assert_allclose(a.item(), b.item(), rtol=RTOL_SCALAR, err_msg=k)
    for k, g in _grads(gp).items():
        assert rel_l2(g.cpu(), og[k]) < REL_L2_GRAD, k


@pytest.mark.parametrize('n_prev', [0, 1])
def test_trainer_graph_step_equals_eager_step(n_prev):
    from vargp_amd import noise, ops
    from vargp_amd.train import ElboTrainer
    S, C, M, D, B = 3, 4, 20, 2, 100
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=303 + n_prev, kind='wtoy')
    nz = {k: v for k, v in nz.items() if k != 'eps_f'}
    y, _ = _targets('labels', C, B, 5)
    xd, yd = x.to(DEV), y.to(DEV)
    ops.set_cholesky_error_mode('defer')
    ops.reset_linalg_errors()
    try:
        results = []
        for mode in ('eager', 'graph'):
            gp = _build(params, prev, S, 'probit')
            tr = ElboTrainer(gp, lr=1e-3, beta=1.0, n_total=float(B))
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
        assert ops.linalg_error_count() == 0
    finally:
        ops.set_cholesky_error_mode('raise')


@pytest.mark.parametrize('shape', [(2, 5, 24, 16, 48, 0), (3, 3, 12, 4, 40, 1), (2, 3, 112, 8, 64, 0)])
def test_retained_graph_second_backward_doubles_the_gradient(shape):
    from vargp_amd import noise
    S, C, M, D, B, n_prev = shape
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=77, kind='gauss')
    nz = {k: v for k, v in nz.items() if k != 'eps_f'}
    y, _ = _targets('labels', C, B, 77)
    res = []
    for twice in (False, True):
        gp = _build(params, prev, S, 'probit')
        with noise.inject(**to_dev(nz, DEV)):
            kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
        loss = 2.0 * kl_h + kl_u + 3.0 * nll
        if twice:
            loss.backward(retain_graph=True)
        loss.backward()
        res.append({k: v.detach().cpu().clone() for k, v in _grads(gp).items()})
    for k in NAMES:
        assert rel_l2(res[1][k], 2 * res[0][k]) < 1e-5, k


@pytest.mark.parametrize('n_prev,D', [(0, 8), (1, 40)])
@pytest.mark.parametrize('link', ['probit', 'logit'])
def test_predict_shape_and_tiled_sweep(n_prev, D, link):
    from vargp_amd import noise
    S, C, M, B = 2, 3, 12, 100
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=41 + n_prev, kind='gauss')
    gp = _build(params, prev, S, link)
    xd = x.to(DEV)
    with noise.inject(eps_theta=nz['eps_theta'].to(DEV)), torch.no_grad():
        one = gp.predict(xd)
        tiled = gp.predict(xd, tile=32)
        mu, var = gp(xd)
    assert one.shape == (B, C) and tiled.shape == (B, C)
    np.testing.assert_allclose(one.cpu().numpy(), rule_probs(mu.cpu().double(), var.cpu().double(), link).numpy(), atol=ATOL_PROBS)
    np.testing.assert_allclose(tiled.cpu().numpy(), one.cpu().numpy(), atol=ATOL_PROBS)


def test_retrain_with_bernoulli_likelihood_vs_fp64_composition(monkeypatch):
    """VARGPRetrain takes the composed route: its fp64 restatement (oracle.retrain_loss) with the rule in place of the softmax."""
    from vargp_amd import noise
    from vargp_amd.vargp_retrain import VARGPRetrain
    S, C, M, D, B, n_prev, seed = 2, 3, 12, 2, 64, 1, 308
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=seed, kind='wtoy')
    Mt = M * (n_prev + 1)
    nz = dict(eps_theta=nz['eps_theta'], eps_u_leq=orc.hash_normal((S, S, C, Mt), seed + 51).float(),
              eps_u_tilde=orc.hash_normal((S, S, S, C, Mt - M), seed + 53).float())
    y, t = _targets('labels', C, B, seed)
    beta, scale = 1.0, 4.0
    monkeypatch.setattr(orc, 'softmax_nll', lambda pmu, pvar, yy, eps_f: rule_nll(pmu, pvar, t, 'probit'))
    d = lambda o: {k: v.double() for k, v in o.items()}
    leaf = d(params)
    for k in NAMES:
        leaf[k] = leaf[k].detach().clone().requires_grad_(True)
    retrain = [{k: v.double().clone().requires_grad_(True) for k, v in p.items()} for p in prev]
    kl_h, kl_u, nll = orc.retrain_loss(leaf, retrain, [d(p) for p in prev], x.double(), y, dict(d(nz), eps_f=None))
    flat = [leaf[k] for k in NAMES] + [p[k] for p in retrain for k in ('z', 'u_mean', 'u_tril_vec')]
    og = torch.autograd.grad(beta * kl_h + kl_u + scale * nll, flat)
    gp = _build(params, prev, S, 'probit', cls=VARGPRetrain)
    with noise.inject(**to_dev(nz, DEV)):
        kh, ku, nl = gp.loss(x.to(DEV), y.to(DEV))
        (beta * kh + ku + scale * nl).backward()
    for a, b, k in [(kh, kl_h, 'kl_hypers'), (ku, kl_u, 'kl_u'), (nl, nll, 'nll')]:
        np.testing.assert_allclose(a.item(), b.item(), rtol=RTOL_SCALAR, err_msg=k)
    got = list(_grads(gp).values()) + [pd[k].grad for pd in gp.retrain_params for k in ('z', 'u_mean', 'u_tril_vec')]
    for i, (a, b) in enumerate(zip(got, og)):
        assert rel_l2(a.cpu(), b) < REL_L2_GRAD, i


# -- refusals: what a Gaussian model is refused, a Bernoulli model is refused ------------------------------------------------------
def test_routes_that_assume_the_softmax_refuse_bernoulli_models(tmp_path):
    import torch.distributed as dist
    from vargp_amd import ops
    from vargp_amd.train import ElboTrainer
    S, C, M, D, B = 3, 4, 20, 2, 100
    params, prev, x, _, _ = orc.make_problem(S, 1, C, M, D, B, n_prev=0, seed=301, kind='wtoy')
    y, _ = _targets('labels', C, B, 1)
    xd, yd = x.to(DEV), y.to(DEV)
    gp = _build(params, prev, S, 'probit')
    assert not gp._lazy_ok()                       # the lazy route: the node route instead
    kl_h, _, _ = gp.loss(xd, yd)
    assert torch.is_tensor(kl_h) and kl_h.grad_fn is not None
    with pytest.raises(NotImplementedError, match='BernoulliLikelihood'):
        gp.elbo_tiled(xd, yd, tile=50)
    ops.set_cholesky_error_mode('defer')
    try:
        tr = ElboTrainer(gp, lr=1e-3)
        tr.capture(xd, yd, warmup=1)
        with pytest.raises(NotImplementedError, match='BernoulliLikelihood'):
            tr.capture_unrolled(xd, yd, 2)
        with pytest.raises(NotImplementedError):
            tr.capture_epoch(xd, yd)
        with pytest.raises(NotImplementedError):
            tr.step_graph_gather(xd, yd, torch.arange(B, device=DEV))
    finally:
        ops.set_cholesky_error_mode('raise')
    own = not dist.is_initialized()
    if own:
        dist.init_process_group('gloo', init_method=f'file://{tmp_path}/pg', rank=0, world_size=1)
    try:
        with pytest.raises(NotImplementedError):
            ElboTrainer(_build(params, prev, S, 'probit'), force_exchange=True)
        with pytest.raises(NotImplementedError):
            ElboTrainer(_build(params, prev, S, 'probit'), force_exchange=True, shards=[(0, 3, 0, 4)])
    finally:
        if own:
            dist.destroy_process_group()


# -- behaviour: two tasks, against the softmax model ------------------------------------------------------------------------------
def _task(t, n, seed):
    """2-D inputs, 3 classes; task 0 lives on x1 in [-2.5, 0], task 1 on [0, 2.5]; the class is the band of x2 + 0.35 sin(2 x1)."""
    gen = torch.Generator().manual_seed(seed)
    x1 = 2.5 * torch.rand(n, generator=gen) - (2.5 if t == 0 else 0.0)
    x2 = 2 * torch.rand(n, generator=gen) - 1
    v = x2 + 0.35 * torch.sin(2 * x1)
    return torch.stack([x1, x2], dim=-1), (v > -0.3).long() + (v > 0.3).long()


def _accuracy(gp, x, y):
    with torch.no_grad():
        return (gp.predict(x.to(DEV)).argmax(-1).cpu() == y).float().mean().item()


def _two_task_run(make_lik):
    from vargp_amd.kernels import RBFKernel
    from vargp_amd.train import ElboTrainer
    from vargp_amd.vargp import VARGP
    torch.manual_seed(0)
    N, B, M, C, steps = 512, 64, 16, 3, 400
    prev, prior, gp = [], (None, None), None
    for t in range(2):
        x, y = _task(t, N, 100 + t)
        z = torch.stack([x[torch.randperm(N)[:M]] for _ in range(C)])
        kern = RBFKernel(2, prior_log_mean=prior[0], prior_log_logvar=prior[1])
        gp = VARGP(z, kern, make_lik(), n_var_samples=2, prev_params=prev).to(DEV)
        tr = ElboTrainer(gp, lr=3e-2, beta=1.0, n_total=N, noise_seed=11 + t)
        xd, yd = x.to(DEV), y.to(DEV)
        for i in range(steps):
            idx = torch.randint(0, N, (B,), device=DEV)
            out = tr.step(xd[idx], yd[idx])
        assert all(torch.isfinite(o).item() for o in out)
        sd = {k: v.detach().clone() for k, v in gp.state_dict().items()}
        prev = prev + [sd]
        prior = (sd['kernel.log_mean'], sd['kernel.log_logvar'])
    return [_accuracy(gp, *_task(t, 1000, 200 + t)) for t in range(2)]


def test_two_task_accuracy_matches_the_softmax_model():
    """After task 1, accuracy on BOTH tasks (1000 held-out points each) is at least the softmax model's minus 0.05 -- about three
    standard errors of an accuracy near 0.9 on 1000 points.  Same loop, steps, learning rate and seeds for both models."""
    from vargp_amd.likelihoods import BernoulliLikelihood, MulticlassSoftmax
    soft = _two_task_run(lambda: MulticlassSoftmax(n_f=10))
    bern = _two_task_run(lambda: BernoulliLikelihood())
    msg = f'softmax: task 0 {soft[0]:.3f}, task 1 {soft[1]:.3f}; bernoulli: task 0 {bern[0]:.3f}, task 1 {bern[1]:.3f}'
    print(msg)
    assert bern[0] >= soft[0] - 0.05 and bern[1] >= soft[1] - 0.05, msg
