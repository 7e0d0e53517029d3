"""GPU: MaternKernel(native=True) models on the native block ELBO program (csrc/elbo_tn.hip with kernel_nu2 = 1 | 3 | 5).

Yardstick: the fp64 restatement of tests/test_hip_matern.py (`matern_ref`, `_oracle_gauss`, imported, not re-derived) patched
into oracle.vargp_oracle.rbf_gram, under the project's sweep rule (tests/sweep_rule.py):

    err(HIP, fp64) <= tolerance + 2 x err(fp32 oracle on one thread, fp64),   RTOL_SCALAR / REL_L2_GRAD of tests/helpers.py.

No tolerance of its own.  Every case asserts that the model DID create a TnProgram and no T0Program: a silent fall-back to the
composed route fails the test.  Shapes of the fixed grid are chosen under sweep_rule.COST_CAP (asserted, never dropped); the
randomised part redraws instead of dropping.
"""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import vargp_oracle as orc
from helpers import ATOL_PRED, REL_L2_GRAD, RTOL_PRED, RTOL_SCALAR, rel_l2, to_dev
from sweep_rule import COST_CAP, _cost, _dbl
from test_hip_matern import BETA, EPS32, NTOT, NUS, _one_thread, _oracle_gauss, matern_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DIRECT_D = 32


def _build(params, prev, S, nu, lik, ep_var_mean=True, native=True, dev=DEV):
    from vargp_amd.kernels import MaternKernel
    from vargp_amd.vargp import VARGP
    D = params['z'].shape[-1]
    kern = MaternKernel(D, nu=nu, prior_log_mean=params['prior_log_mean'], prior_log_logvar=params['prior_log_logvar'],
                        native=native)
    gp = VARGP(params['z'], kern, lik, n_var_samples=S, ep_var_mean=ep_var_mean,
               prev_params=[{k: v.clone() for k, v in p.items()} for p in prev])
    with torch.no_grad():
        gp.kernel.log_mean.copy_(params['log_mean'])
        gp.kernel.log_logvar.copy_(params['log_logvar'])
        gp.u_mean.copy_(params['u_mean'])
        gp.u_tril_vec.copy_(params['u_tril_vec'])
    return gp.to(dev)


def _on_block_program(gp, training=True):
    """The model ran natively: a TnProgram with the Matern code exists, and no first-task program (csrc/elbo_t0.hip is RBF-only)."""
    from vargp_amd.fused import TnProgram
    from vargp_amd.kernels import native_code
    assert not gp._t0_progs and not gp._t0_spares, 'a native Matern model created a T0Program'
    progs = list(gp._tn_progs.values()) if training else [p for p in [gp._tn_eval, *gp._tn_eval_exact.values()] if p is not None]
    assert progs and all(type(p) is TnProgram and p.kernel_nu2 == native_code(gp.kernel) and p.desc.kernel_nu2 == p.kernel_nu2
                         for p in progs), f'no native block program on the model: {progs}'


def _grads(gp):
    return [p.grad.detach().cpu().double() for p in (gp.z, gp.u_mean, gp.u_tril_vec, gp.kernel.log_mean, gp.kernel.log_logvar)]


def _tile_of(Mg, Ng, nbatch, tri):
    """launch_gemm_epi's tile rule (csrc/gemm.hip) for a distance product [Mg x Ng], for the log."""
    cd = lambda a, b: -(-a // b)
    t128, t12864 = cd(Mg, 128) * cd(Ng, 128) * nbatch, cd(Mg, 128) * cd(Ng, 64) * nbatch
    pad64_less = cd(Mg, 64) * 64 < cd(Mg, 128) * 128
    if t12864 >= 384 and tri and pad64_less:
        return '64x64x64'
    if t128 >= 512 and not tri and Mg >= 1024 and Ng >= 1024:
        return '128x128x16'
    if t12864 >= 384 and Mg > 64:
        return '128x64x32'
    return '64x64x64'


def _forms(c):
    Mt = c['M'] * (c['n_prev'] + 1)
    if c['D'] <= DIRECT_D:
        return 'direct'
    return 'gemm K_all %s, K_uf %s' % (_tile_of(Mt, Mt, c['S'] * c['C'], True), _tile_of(c['C'] * Mt, c['B'], c['S'], False))


def _problem(c, nu, coincident=False):
    from vargp_amd.likelihoods import MulticlassSoftmax
    S, F_, C, M, D, B, n_prev = (c[k] for k in ('S', 'F', 'C', 'M', 'D', 'B', 'n_prev'))
    kind = c.get('kind') or ('wtoy' if D == 2 else 'gauss')
    params, prev, x, y, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=n_prev, seed=c['seed'], kind=kind)
    # prev_params as earlier Matern tasks leave them: z, u_mean, u_tril_vec of a state dict
    out = []
    for p in prev:
        first = _build(dict(params, **p), [], S, nu, MulticlassSoftmax(n_f=F_), dev='cpu')
        out.append({k: v.detach().clone() for k, v in first.state_dict().items() if k in ('z', 'u_mean', 'u_tril_vec')})
    if coincident:      # what create_clf produces on purpose: inducing points ARE data points
        x = x.clone()
        x[:M] = params['z'][0]
        x[M:2 * M] = params['z'][-1]
    return params, out, x, y, nz


def _case(c, nu, lik='softmax', coincident=False, monkeypatch=None, label='grid'):
    """One case under the sweep rule -> ((err / bound, quantity, err, bound) of the worst quantity, tag)."""
    from vargp_amd import noise
    from vargp_amd.likelihoods import GaussianLikelihood, MulticlassSoftmax
    assert _cost(c['S'], c['C'], c['M'], c['n_prev'], c['D'], c['B']) <= COST_CAP, c
    monkeypatch.setattr(orc, 'rbf_gram', lambda theta, x, y=None, full_gram=False: matern_ref(theta, x, y, nu=nu))
    S, F_, C, B, nomean = c['S'], c['F'], c['C'], c['B'], c['nomean']
    params, prev, x, y, nz = _problem(c, nu, coincident)
    if lik == 'gauss':
        nz = {k: v for k, v in nz.items() if k != 'eps_f'}
        y = torch.sin(3.0 * x.sum(-1, keepdim=True).T + torch.arange(C).view(C, 1)).float()
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
    _on_block_program(gp)
    sc = dict(kl_hypers=float(kl_h), kl_u=float(kl_u), nll=float(nll))
    gr = dict(z=gp.z.grad, u_mean=gp.u_mean.grad, u_tril_vec=gp.u_tril_vec.grad, log_mean=gp.kernel.log_mean.grad,
              log_logvar=gp.kernel.log_logvar.grad)
    if lik == 'gauss':
        gr['obs_log_var'] = gp.likelihood.obs_log_var.grad
    gr = {k: v.detach().cpu().double() for k, v in gr.items()}
    gp.release_programs()
    rel = lambda a, b: abs(a - b) / abs(b)
    e_sc = {k: (rel(v, s64[k].item()), rel(s32[k].item(), s64[k].item())) for k, v in sc.items() if s64[k].item() != 0.0}
    e_gr = {'grad ' + k: (rel_l2(g, g64[k]), rel_l2(g32[k].double(), g64[k])) for k, g in gr.items()}
    worst = (0.0, None, 0.0, 0.0)
    for errs, tol in ((e_sc, RTOL_SCALAR), (e_gr, REL_L2_GRAD)):
        bound = tol + 2.0 * max(b for _, b in errs.values())
        for k, (a, _) in errs.items():
            if a / bound > worst[0]:
                worst = (a / bound, k, a, bound)
    tag = 'nu={nu} S{S} F{F} C{C} M{M} t{n_prev} D{D} B{B} nomean={nm} {lik} seed={seed}'.format(
        nu=nu, nm=int(nomean), lik=lik, **{k: v for k, v in c.items() if k not in ('nomean', 'kind')})
    print(f'[{label}] {tag} ({_forms(c)}): worst {worst[1]} err {worst[2]:.2e} (bound {worst[3]:.2e})', flush=True)
    return worst, tag


# -- fixed grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('n_prev', [0, 1, 2])
@pytest.mark.parametrize('nomean', [False, True])
@pytest.mark.parametrize('lik', ['softmax', 'gauss'])
@pytest.mark.parametrize('D', [2, 24, 40, 784])
def test_model_loss_and_grads_vs_oracle(nu, n_prev, nomean, lik, D, monkeypatch):
    """nu x {first task, 1, 2 earlier tasks} x ep_var_mean x likelihood x D (2, 24: direct form; 40, 784: GEMM)."""
    c = dict(S=2, F=3, C=3, M=12, n_prev=n_prev, D=D, B=48, nomean=nomean, seed=3 + int(2 * nu) + 10 * n_prev + D,
             kind='mnist' if D == 784 else None)
    worst, tag = _case(c, nu, lik, monkeypatch=monkeypatch)
    assert worst[0] <= 1.0, (tag, worst)


# M not a multiple of 4 / of 16, M > 104 (several panels of the blocked factorisation), B not a multiple of 64, and the two
# GEMM tiles a distance product of the program can take under COST_CAP (64x64x64; 128x64x32 for K_uf from 384 tiles of
# 128 x 64 on; 128x128x16 needs both extents >= 1024 in >= 512 tiles, beyond the cap)
EDGE_CASES = [
    dict(S=2, F=2, C=3, M=13, n_prev=1, D=40, B=100, nomean=False, seed=501),
    dict(S=2, F=2, C=2, M=22, n_prev=2, D=24, B=70, nomean=True, seed=502),
    dict(S=2, F=2, C=2, M=112, n_prev=0, D=40, B=130, nomean=False, seed=503),
    dict(S=1, F=2, C=2, M=120, n_prev=1, D=784, B=65, nomean=False, seed=504, kind='mnist'),
    dict(S=5, F=1, C=10, M=128, n_prev=0, D=40, B=512, nomean=False, seed=505),
    dict(S=3, F=10, C=10, M=100, n_prev=0, D=784, B=512, nomean=False, seed=506, kind='mnist'),
]


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('ci', range(len(EDGE_CASES)))
def test_edge_shapes_vs_oracle(nu, ci, monkeypatch):
    worst, tag = _case(EDGE_CASES[ci], nu, monkeypatch=monkeypatch, label='edge')
    assert worst[0] <= 1.0, (tag, worst)


def test_edge_shapes_cover_both_tiles():
    forms = [_forms(c) for c in EDGE_CASES]
    assert any('K_uf 128x64x32' in f for f in forms) and any('K_uf 64x64x64' in f for f in forms) and any(f == 'direct' for f in forms)


# -- randomised sweep ---------------------------------------------------------------------------------------------------------------
N_RANDOM = 24


def _random_cases(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:                     # redraw, never drop
        S, C, F_ = int(rng.integers(1, 5)), int(rng.integers(1, 7)), int(rng.integers(1, 4))
        M = int(rng.choice([4, 8, 13, 20, 30, 33, 52, 64, 77, 100, 104, 108, 120]))
        n_prev = int(rng.integers(0, 4))
        D = int(rng.choice([2, 4, 8, 24, 32, 33, 36, 40, 64, 784]))
        B = int(rng.choice([8, 30, 36, 64, 65, 68, 128, 200]))
        nomean = bool(rng.integers(0, 4) == 0)
        if _cost(S, C, M, n_prev, D, B) > COST_CAP / 4:
            continue
        out.append(dict(S=S, F=F_, C=C, M=M, n_prev=n_prev, D=D, B=B, nomean=nomean, seed=700 + len(out) + seed))
    return out


@pytest.mark.parametrize('nu', NUS)
def test_random_shapes_vs_oracle(nu, monkeypatch):
    rows = [_case(c, nu, monkeypatch=monkeypatch, label='random') for c in _random_cases(N_RANDOM, int(20 * nu))]
    bad = [(tag, w) for w, tag in rows if w[0] > 1.0]
    w = max(rows, key=lambda r: r[0][0])
    print(f'[random nu={nu}] {len(rows)} cases; worst {w[1]}: {w[0][1]} at {w[0][0]:.2f} of its bound')
    assert len(rows) == N_RANDOM and not bad, bad


# -- coincident points --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('D', [2, 40])
def test_coincident_points(nu, D, monkeypatch):
    """z rows copied into x.  nu = 3/2, 5/2 (and nu = 1/2 in the direct form, where the copies' distance is exactly 0): the sweep
    rule against fp64.  nu = 1/2 in the GEMM form: d2 of a copied pair is rounding noise where fp64 has 0, so K there is within
    test_hip_matern.test_coincident_points' bound of gamma^2 (|1 - k / g2| <= sqrt(2 nu 4 D eps na) + 4 eps), checked on the
    K_uf the program's moments are built from -- the op's, same epilogue -- and the program must agree with the composed route
    of the same build (same clamp, same derivative at 0): a consistency check on top, not the yardstick."""
    from vargp_amd import noise, ops
    from vargp_amd.likelihoods import MulticlassSoftmax
    c = dict(S=2, F=3, C=3, M=12, n_prev=1, D=D, B=48, nomean=False, seed=90 + D)
    if not (nu == 0.5 and D > DIRECT_D):
        worst, tag = _case(c, nu, coincident=True, monkeypatch=monkeypatch, label='coincident')
        assert worst[0] <= 1.0, (tag, worst)
        return
    params, prev, x, y, nz = _problem(c, nu, coincident=True)
    S, M = c['S'], c['M']
    theta = params['log_mean'].unsqueeze(0) + nz['eps_theta'] * (0.5 * params['log_logvar']).exp().unsqueeze(0)
    K = ops.matern_gram(theta.to(DEV), params['z'].to(DEV), x.to(DEV), True, nu).cpu()
    g2 = (2.0 * theta[:, -1].double()).exp()
    na = ((params['z'][0].double().unsqueeze(0) / theta[:, :-1].double().exp().view(S, 1, D)) ** 2).sum(-1)      # (S, M)
    dev = (1.0 - K[:, 0, torch.arange(M), torch.arange(M)].double() / g2.view(S, 1)).abs()
    bound = (2 * nu * 4 * D * EPS32 * na).sqrt() + 4 * EPS32
    print('copied pairs: worst deviation %.2e, bound there %.2e' % (dev.max().item(), bound.flatten()[dev.argmax()].item()))
    assert (dev <= bound).all()
    res = []
    for native in (True, False):
        gp = _build(params, prev, S, nu, MulticlassSoftmax(n_f=c['F']), native=native)
        with noise.inject(**to_dev(nz, DEV)):
            out = gp.loss(x.to(DEV), y.to(DEV))
            (BETA * out[0] + out[1] + NTOT * out[2]).backward()
        if native:
            _on_block_program(gp)
        else:
            assert not gp._tn_progs and not gp._t0_progs
        res.append(([float(v) for v in out], _grads(gp)))
    (s_n, g_n), (s_c, g_c) = res
    print('native vs composed: scalars', [abs(a - b) / abs(b) for a, b in zip(s_n, s_c)], 'grads', [rel_l2(a, b) for a, b in zip(g_n, g_c)])
    for a, b in zip(s_n, s_c):
        assert abs(a - b) <= RTOL_SCALAR * abs(b)
    for a, b in zip(g_n, g_c):
        assert torch.isfinite(a).all() and rel_l2(a, b) <= REL_L2_GRAD


# -- routes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('n_prev', [0, 1])
def test_lazy_route_equals_autograd_node(nu, n_prev):
    """Same inputs through lazy terms and through one autograd node: equal to the run-to-run spread of the float atomics
    (gtheta, the r / c sums, the KL and nll scalars): 64 eps32 of the norm, as test_hip_matern allows for such sums."""
    from vargp_amd import noise
    from vargp_amd.likelihoods import MulticlassSoftmax
    c = dict(S=2, F=3, C=3, M=20, n_prev=n_prev, D=40, B=64, nomean=False, seed=61)
    params, prev, x, y, nz = _problem(c, nu)
    res = []
    for lazy in (True, False):
        gp = _build(params, prev, c['S'], nu, MulticlassSoftmax(n_f=c['F']))
        gp.lazy_loss = lazy
        with noise.inject(**to_dev(nz, DEV)):
            out = gp.loss(x.to(DEV), y.to(DEV))
            assert type(out[0]).__module__.endswith('lazy') == lazy
            (BETA * out[0] + out[1] + NTOT * out[2]).backward()
        _on_block_program(gp)
        res.append(([float(v) for v in out], _grads(gp)))
    (s_l, g_l), (s_n, g_n) = res
    np.testing.assert_allclose(s_l, s_n, rtol=64 * EPS32)
    for a, b in zip(g_l, g_n):
        assert rel_l2(a, b) <= 64 * EPS32


@pytest.mark.parametrize('nu', NUS)
def test_elbo_tiled_equals_one_loss(nu):
    """N = 3 full tiles + a ragged one against one loss() on all N (injected noise): values and gradients."""
    from vargp_amd import noise
    from vargp_amd.likelihoods import MulticlassSoftmax
    tile, N = 64, 3 * 64 + 23
    c = dict(S=2, F=2, C=3, M=20, n_prev=1, D=40, B=N, nomean=False, seed=71)
    params, prev, x, y, nz = _problem(c, nu)
    res = []
    for tiled in (True, False):
        gp = _build(params, prev, c['S'], nu, MulticlassSoftmax(n_f=c['F']))
        with noise.inject(**to_dev(nz, DEV)):
            if tiled:
                out = gp.elbo_tiled(x.to(DEV), y.to(DEV), tile, beta=BETA, scale=NTOT)
            else:
                out = gp.loss(x.to(DEV), y.to(DEV))
                (BETA * out[0] + out[1] + NTOT * out[2]).backward()
        _on_block_program(gp)
        res.append(([float(v) for v in out], _grads(gp)))
    (s_t, g_t), (s_o, g_o) = res
    print('tiled vs one call:', [abs(a - b) / abs(b) for a, b in zip(s_t, s_o)], [rel_l2(a, b) for a, b in zip(g_t, g_o)])
    np.testing.assert_allclose(s_t, s_o, rtol=RTOL_SCALAR)
    for a, b in zip(g_t, g_o):
        assert rel_l2(a, b) <= REL_L2_GRAD


@pytest.mark.parametrize('nu', NUS)
@pytest.mark.parametrize('n_prev,D', [(0, 8), (1, 40)])
def test_predict_tiled_and_forward_only_program(nu, n_prev, D):
    """predict(x, tile=) == predict(x) (GaussianLikelihood: the means draw nothing but eps_theta), and the forward-only
    program's moments == the training program's (its likelihood buffers after a loss on the same inputs)."""
    from vargp_amd import fused, noise
    from vargp_amd.likelihoods import GaussianLikelihood
    S, C, M, B = 2, 3, 12, 100
    c = dict(S=S, F=1, C=C, M=M, n_prev=n_prev, D=D, B=B, nomean=False, seed=41 + n_prev)
    params, prev, x, _, nz = _problem(c, nu)
    gp = _build(params, prev, S, nu, GaussianLikelihood(C))
    xd = x.to(DEV)
    with noise.inject(eps_theta=nz['eps_theta'].to(DEV)), torch.no_grad():
        one = gp.predict(xd)
        tiled = gp.predict(xd, tile=32)
        mu_f, var_f = gp(xd)
    _on_block_program(gp, training=False)
    np.testing.assert_allclose(tiled.cpu().numpy(), one.cpu().numpy(), rtol=RTOL_PRED, atol=ATOL_PRED)
    with noise.inject(eps_theta=nz['eps_theta'].to(DEV)):
        gp.loss(xd, torch.zeros(C, B, device=DEV))
    _on_block_program(gp)
    mu_t, var_t, _, _ = fused.lik_views(next(iter(gp._tn_progs.values())))
    np.testing.assert_allclose(mu_f.cpu().numpy(), mu_t.cpu().numpy(), rtol=RTOL_PRED, atol=ATOL_PRED)
    np.testing.assert_allclose(var_f.cpu().numpy(), var_t.cpu().numpy(), rtol=RTOL_PRED, atol=ATOL_PRED)


# -- trainer ------------------------------------------------------------------------------------------------------------------------
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
            assert tr._tn and type(tr._prog).__name__ == 'TnProgram' and tr._prog.kernel_nu2 == int(2 * nu)
            assert not gp._t0_progs
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
    """Native noise (the program's own generator), eager steps."""
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.train import ElboTrainer
    S, F_, C, M, D, B = 2, 4, 4, 12, 2, 128
    params, prev, x, _, _ = orc.make_problem(S, F_, C, M, D, B, n_prev=0, seed=21, kind='wtoy')
    y = ((x[:, 0] > 0).long() + 2 * (x[:, 1] > 0).long())
    gp = _build(params, prev, S, nu, MulticlassSoftmax(n_f=F_))
    tr = ElboTrainer(gp, lr=1e-2, beta=1.0, n_total=B)
    assert tr.native_noise
    xd, yd = x.to(DEV), y.to(DEV)
    torch.manual_seed(0)
    totals = []
    for _ in range(200):
        kl_h, kl_u, nll = (float(v) for v in tr.step(xd, yd))
        totals.append(kl_h + kl_u + nll)
    assert tr._tn and tr._prog.kernel_nu2 == int(2 * nu) and not gp._t0_progs
    first, last = np.mean(totals[:10]), np.mean(totals[-10:])
    print('toy run nu=%s: loss %.4f -> %.4f' % (nu, first, last))
    assert np.isfinite(totals).all() and last < first


@pytest.mark.parametrize('mode', ['raise', 'defer', 'lazy'])
def test_cholesky_error_modes(mode):
    """A healthy native Matern step in each of the three Cholesky error modes: no error noted, finite results."""
    from vargp_amd import noise, ops
    from vargp_amd.likelihoods import MulticlassSoftmax
    c = dict(S=2, F=2, C=3, M=12, n_prev=1, D=40, B=48, nomean=False, seed=5)
    params, prev, x, y, nz = _problem(c, 1.5)
    ops.set_cholesky_error_mode(mode)
    ops.reset_linalg_errors()
    try:
        gp = _build(params, prev, c['S'], 1.5, MulticlassSoftmax(n_f=c['F']))
        with noise.inject(**to_dev(nz, DEV)):
            out = gp.loss(x.to(DEV), y.to(DEV))
            sum(out).backward()
        torch.cuda.synchronize()
        ops.check_linalg_errors()
        _on_block_program(gp)
        assert all(math.isfinite(float(v)) for v in out) and ops.linalg_error_count() == 0
    finally:
        ops.set_cholesky_error_mode('raise')


# -- two sample-parallel ranks on one GPU (as tests/test_hip_dist.py) ---------------------------------------------------------------
S_LOCAL, WORLD, SEED = 2, 2, 31


def _dist_model(S, dev='cuda:0'):
    from vargp_amd.kernels import MaternKernel
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.synthetic import mnist_like
    from vargp_amd.vargp import VARGP
    F_, C, M, D, B = 4, 4, 12, 40, 64
    torch.manual_seed(0)
    xall, yall = mnist_like(1024, D, C, kind='gauss', seed=1)
    z = torch.stack([xall[yall == c][:M] for c in range(C)])
    gp = VARGP(z, MaternKernel(D, nu=1.5, native=True), MulticlassSoftmax(n_f=F_), n_var_samples=S).to(dev)
    return gp, xall[:B].to(dev), yall[:B].to(dev)


def _dist_steps(gp, x, y):
    from vargp_amd.train import ElboTrainer
    tr = ElboTrainer(gp, lr=1e-3, beta=2.0, n_total=10 * x.shape[0], noise_seed=SEED)
    outs = [[o.item() for o in tr.step(x, y)] for _ in range(3)]
    torch.cuda.synchronize()
    assert tr._tn and tr._prog.kernel_nu2 == 3 and not gp._t0_progs
    return outs, {k: v.detach().cpu().numpy() for k, v in gp.state_dict().items()}


def _dist_worker(rank, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(WORLD))
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', rank=rank, world_size=WORLD)
    try:
        from vargp_amd import ops
        ops.set_cholesky_error_mode('defer')
        outs, sd = _dist_steps(*_dist_model(S_LOCAL))
        if rank == 0:
            q.put((outs, sd))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_equal_single_process():
    from vargp_amd import noise, ops
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_worker, args=(r, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    outs2, sd2 = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    ops.set_cholesky_error_mode('defer')
    try:
        outs1, sd1 = _dist_steps(*_dist_model(S_LOCAL * WORLD))
    finally:
        noise.clear_shard()
        ops.set_cholesky_error_mode('raise')
    np.testing.assert_allclose(np.array(outs2), np.array(outs1), rtol=2e-4)
    for k in sd1:
        err = np.linalg.norm(sd2[k] - sd1[k]) / max(np.linalg.norm(sd1[k]), 1e-30)
        assert err < 1e-4, (k, err)
