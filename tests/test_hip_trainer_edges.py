"""GPU: the route `ElboTrainer` takes through the first-task program -- the softmax likelihood and its gradient evaluated inside
the backward's tile kernel (`defer_softmax`: t0_bwd_mid.h, the `sm.eps` branch), the theta gradient finished inside the Yogi launch
(`defer_hyper`), by default noise drawn by the program itself -- against the oracle in fp64, at the edges of that code: one wave
per four likelihood samples (F = 1, 4, 5, 13, 16 and the fall-back at 17), classes in groups of four up to 16 (C = 1, 3, 4, 5,
10, 16 and the generic likelihood at 17), a ragged last 64-column tile, and every launch sequence the plan (T0Plan,
csrc/elbo_t0.hip) can put around it.  Every case first asserts the plan the trainer's own program reports
(`T0Program.plan()`: the library's t0_plan on the descriptor of that step), so a retuned threshold that moves a shape to another
path fails here instead of silently testing something else; tests/test_t0_plan.py asserts the same flags without a GPU at 256
CUs and holds the list to a coverage condition.

Tolerances: helpers.RTOL_SCALAR for the loss terms, helpers.REL_L2_GRAD per gradient tensor; where the oracle in fp32 (one host
thread) misses one of them itself, the rule of tests/sweep_rule.py for that class: tolerance + 2 x the fp32 oracle's error.
Two routes of the same arithmetic (deferred against undeferred likelihood): 1e-5, as test_hip_train.test_graph_step_equals_eager_step.
Every case prints its errors (pytest -s).

Measured on an MI355X (256 CUs; the plan the program reported there, flags that are on besides unscaled_lik_grad / generic_lik and
w_vec4; worst loss term / worst gradient against fp64 -- the worst gradient is always z):
  (1, 1, 1, 4, 36, 4)       defer_softmax fused_mid fused_bwd mat_bwd fused_tail fold_small                          2.5e-7 / 1.5e-7
  (2, 4, 4, 20, 36, 64)     the same                                                                                 1.0e-7 / 5.1e-7
  (2, 5, 3, 36, 40, 72)     the same, two tiles                                                                      9.3e-8 / 5.9e-7
  (1, 13, 16, 52, 36, 132)  the same + merge_chol, three tiles                                                       3.3e-8 / 1.0e-6
  (2, 16, 5, 68, 256, 64)   the same + split_kuu front su_in_chain                                                   4.8e-8 / 6.7e-7
  (3, 10, 10, 100, 256, 72) the same, two tiles                                                                      4.8e-8 / 7.5e-7
  (9, 2, 10, 68, 256, 64)   defer_softmax merge_chol split_kuu front gram_in_chain su_in_chain fused_mid unmerge side
                            fused_bwd mat_bwd fused_tail tail_lds                                                    8.8e-8 / 5.1e-7
  (65, 1, 2, 52, 36, 40)    defer_softmax merge_chol fused_mid unmerge side fused_bwd                                2.1e-7 / 2.4e-7
  (3, 2, 2, 52, 38, 40)     defer_softmax fused_mid fused_bwd fold_small                                             1.2e-7 / 5.5e-7
  (2, 8, 2, 20, 8, 64)      defer_softmax direct_gram fused_mid fused_bwd mat_bwd fused_tail fold_small              3.8e-7 / 3.5e-6
  (2, 17, 3, 36, 40, 64)    fwd_softmax16 fused_mid fused_bwd mat_bwd fused_tail fold_small                          9.4e-8 / 5.4e-7
  (2, 3, 17, 20, 36, 64)    generic_lik fused_mid fused_bwd mat_bwd fused_tail fold_small                            4.2e-8 / 4.9e-7
  (3, 2, 3, 33, 40, 64)     fwd_softmax16 only                                                                       9.3e-8 / 4.8e-7
  (2, 3, 3, 36, 40, 50)     fwd_softmax16 fused_mid, no w_vec4                                                       9.3e-8 / 5.7e-7
  (6, 2, 10, 52, 36, 328)   fwd_softmax16 merge_chol fused_mid fwd_multi fused_bwd mat_bwd bwd_multi fused_tail tail_lds,
                            six tiles on three workgroups                                                            2.8e-7 / 6.0e-7
  (1, 3, 3, 24, 40, 32) map defer_softmax fused_mid fused_bwd mat_bwd fused_tail fold_small                          8.2e-8 / 5.0e-7
Native noise (plans as above + native): <= 1.6e-7 / 6.1e-7; graph replay: <= 3.3e-8 / 1.0e-6; deferred against undeferred
likelihood: <= 9.5e-7 over all gradients, nll within 2e-7.  The fp32 oracle met both tolerances on every shape, so no
bound was widened."""
import numpy as np
import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import rel_l2, to_dev, RTOL_SCALAR, REL_L2_GRAD, GRAD_KEYS
from sweep_rule import _dbl

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 43
BETA = 2.0
SCALARS = ('kl_hypers', 'kl_u', 'nll')

# ((S, F, C, M, D, B), map_est, flags the plan must show on a 256-CU device: 'name' true, '!name' false)
EDGES = [
    # every dimension at its minimum; C = 1: every tile workgroup is the one that adds the nll (cme == 0)
    ((1, 1, 1, 4, 36, 4), False, 'defer_softmax mat_bwd'),
    # exactly one full wave of likelihood samples, one full group of classes
    ((2, 4, 4, 20, 36, 64), False, 'defer_softmax'),
    # a second wave with one live sample, a ragged tile of 8 columns
    ((2, 5, 3, 36, 40, 72), False, 'defer_softmax'),
    # four waves, the last a quarter full; C at the limit kBmSmC = 16; three tiles, the last 4 columns wide
    ((1, 13, 16, 52, 36, 132), False, 'defer_softmax merge_chol'),
    # F at the limit 4 kBmSmF = 16, C no multiple of 4; behind the front launch
    ((2, 16, 5, 68, 256, 64), False, 'defer_softmax front su_in_chain'),
    # the benchmark's launch sequence at its smallest D, with a ragged tile
    ((3, 10, 10, 100, 256, 72), False, 'defer_softmax front fold_small'),
    # the role-merged launches taken apart, Gram matrices by the chain workgroups, the LDS-staged tail
    ((9, 2, 10, 68, 256, 64), False, 'defer_softmax unmerge gram_in_chain tail_lds'),
    # the tile kernels without the per-matrix chains: S > kTailSMax (launches taken apart), and D % 4 != 0
    ((65, 1, 2, 52, 36, 40), False, 'defer_softmax unmerge !mat_bwd'),
    ((3, 2, 2, 52, 38, 40), False, 'defer_softmax !mat_bwd'),
    # the direct distance form (D = 8: D = 2 with M = 20 is ill-conditioned, test_hip_t0_program.py)
    ((2, 8, 2, 20, 8, 64), False, 'defer_softmax direct_gram'),
    # F past the limit: the forward's own softmax launch in front of the LDS-resident backward
    ((2, 17, 3, 36, 40, 64), False, '!defer_softmax fwd_softmax16 fused_bwd'),
    # C past the limit: the generic likelihood
    ((2, 3, 17, 20, 36, 64), False, 'generic_lik !defer_softmax'),
    # M % 4 != 0 and B % 4 != 0: no LDS-resident backward at all
    ((3, 2, 3, 33, 40, 64), False, '!fused_bwd'),
    ((2, 3, 3, 36, 40, 50), False, '!fused_bwd'),
    # more tile units than CUs: the multi-tile backward keeps the softmax launch
    ((6, 2, 10, 52, 36, 328), False, 'bwd_multi !defer_softmax'),
    # MAP estimate of the hyper-parameters
    ((1, 3, 3, 24, 40, 32), True, 'defer_softmax'),
]
IDS = ['%s%s' % (s, '-map' if m else '') for s, m, _ in EDGES]
DEFERRED = [e for e in EDGES if 'defer_softmax' in e[2].split()]
NATIVE = [e for e in EDGES if e[0] in ((2, 5, 3, 36, 40, 72), (2, 16, 5, 68, 256, 64), (9, 2, 10, 68, 256, 64))]
GRAPH = [e for e in EDGES if e[0] in ((1, 13, 16, 52, 36, 132), (9, 2, 10, 68, 256, 64))]
LOSS_NATIVE = (2, 5, 3, 36, 40, 72)           # test_loss_route_native_noise_vs_fp64
_ids = lambda cases: ['%s%s' % (s, '-map' if m else '') for s, m, _ in cases]


def flags_of(text):
    """'a !b' -> {'a': True, 'b': False}"""
    return {w.lstrip('!'): not w.startswith('!') for w in text.split()}


def _assert_plan(plan, want, what):
    bad = {k: v for k, v in flags_of(want).items() if plan[k] != v}
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert not bad, f'{what}: the plan on this device ({cus} CUs) does not show {bad}: {plan}'


# -- problems and oracles: once per case, shared, never modified ---------------------------------------------------------------
_PROBLEM, _ORACLE = {}, {}


def _problem(shape):
    if shape not in _PROBLEM:
        S, F_, C, M, D, B = shape
        _PROBLEM[shape] = orc.make_problem(S, F_, C, M, D, B, n_prev=0, seed=SEED)
    return _PROBLEM[shape]


def _oracles(shape, map_est, nz):
    """-> ((scalars, grads) of the oracle in fp32 on one host thread, the same in fp64) with beta = 2, n_total = 7 B.
    map_est: theta = log_mean (no hyper-parameter noise), no hyper-KL -- neither in the value nor in the gradient of log_mean."""
    params, prev, x, y, _ = _problem(shape)
    nz = dict(nz)
    kw = dict(beta=BETA, n_total=7 * shape[5])
    if map_est:
        nz['eps_theta'] = torch.zeros(1, shape[4] + 1)
        kw['beta'] = 0.0
    n_threads = torch.get_num_threads()
    torch.set_num_threads(1)          # (sweep_rule.oracle_pair: the fp32 error must not depend on the host's thread count)
    try:
        r32 = orc.elbo_step(params, prev, x, y, nz, **kw)
    finally:
        torch.set_num_threads(n_threads)
    r64 = orc.elbo_step(_dbl(params), _dbl(prev), _dbl(x), y, _dbl(nz), **kw)
    return r32, r64


def _oracle(shape, map_est):
    if (shape, map_est) not in _ORACLE:
        _ORACLE[shape, map_est] = _oracles(shape, map_est, _problem(shape)[4])
    return _ORACLE[shape, map_est]


# -- one step of the trainer ---------------------------------------------------------------------------------------------------
def _trainer_step(shape, map_est, graph=False, native=False):
    """One step of ElboTrainer (its defaults) -> (trainer, scalars, gradients as that step left them in the trainer's buffers,
    the noise of the step).  native: the program draws the noise itself; it is read back from the program's workspace."""
    from vargp_amd import noise, ops
    from vargp_amd.train import ElboTrainer
    from gpu_common import build_gp
    S, F_, C, M, D, B = shape
    params, prev, x, y, nz = _problem(shape)
    gp = build_gp(params, prev, S, F_)
    gp.kernel.map_est = map_est
    xd, yd = x.to(DEV), y.to(DEV)
    ops.set_cholesky_error_mode('defer' if graph else 'raise')
    ops.reset_linalg_errors()
    try:
        # lr tiny: the parameter update must not be what is measured; the gradients are read from the buffers
        tr = ElboTrainer(gp, lr=1e-9, beta=BETA, n_total=7 * B, **(dict(noise_seed=4711) if native else {}))
        inj = {} if native else {k: v.contiguous() for k, v in to_dev(nz, DEV).items() if not (map_est and k == 'eps_theta')}
        with noise.inject(**inj):
            if graph:
                tr.capture(xd, yd)
                out = tr.step_graph()
            else:
                out = tr.step(xd, yd)
            torch.cuda.synchronize()
            sc = dict(zip(SCALARS, (float(v) for v in out)))
        k = gp.kernel
        grads = dict(z=gp.z.grad, u_mean=gp.u_mean.grad, u_tril_vec=gp.u_tril_vec.grad, log_mean=k.log_mean.grad,
                     log_logvar=None if map_est else k.log_logvar.grad)
        grads = {n: g.detach().clone().cpu() for n, g in grads.items() if g is not None}
        if graph:
            assert ops.linalg_error_count() == 0
    finally:
        ops.set_cholesky_error_mode('raise')
    assert tr._t0 and not tr._tn and tr._defer_hyper()
    if native:
        prog = tr._prog
        nz = dict(eps_f=prog.eps_f().detach().clone().cpu())
        if not map_est:
            nz['eps_theta'] = prog.eps_theta().detach().clone().cpu()
    return tr, sc, grads, nz


def _check_against_oracle(tag, sc, grads, r32, r64, map_est=False):
    """Per class (loss terms by relative error, gradients by relative L2): the tolerance -- or, where the fp32 oracle itself
    misses it, tolerance + 2 x the fp32 oracle's error (tests/sweep_rule.py)."""
    (s32, g32), (s64, g64) = r32, r64
    if map_est:
        assert sc['kl_hypers'] == 0.0 and 'log_logvar' not in grads
    names = [k for k in SCALARS if not (map_est and k == 'kl_hypers')]
    # (a term that is exactly 0 in fp64 -- the nll of a one-class softmax -- is held to the tolerance as an absolute error)
    e_sc = {k: (abs(sc[k] - s64[k].item()) / (abs(s64[k].item()) or 1.0), abs(s32[k].item() - s64[k].item()) / (abs(s64[k].item()) or 1.0))
            for k in names}
    e_gr = {'grad ' + k: (rel_l2(grads[k], g64[k]), rel_l2(g32[k].double(), g64[k])) for k in GRAD_KEYS if k in grads}
    bad = []
    for errs, tol in ((e_sc, RTOL_SCALAR), (e_gr, REL_L2_GRAD)):
        e32 = max(e for _, e in errs.values())
        bound = tol + (2.0 * e32 if e32 > tol else 0.0)
        for k, (e_hip, e_32) in errs.items():
            print(f'{tag} {k}: hip {e_hip:.2e}  fp32 oracle {e_32:.2e}  bound {bound:.2e}', flush=True)
            if not e_hip <= bound:
                bad.append((k, e_hip, bound))
    assert not bad, (tag, bad)


# -- the tests -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,map_est,want', EDGES, ids=IDS)
def test_trainer_step_matches_fp64_oracle(shape, map_est, want):
    tr, sc, grads, _ = _trainer_step(shape, map_est)
    plan = tr._prog.plan()
    print(shape, 'plan:', plan)
    _assert_plan(plan, want + ' !native', shape)
    _check_against_oracle(str(shape), sc, grads, *_oracle(shape, map_est), map_est=map_est)


@pytest.mark.parametrize('shape,map_est,want', DEFERRED, ids=_ids(DEFERRED))
def test_deferred_likelihood_equals_the_forward_launch(shape, map_est, want, monkeypatch):
    """The same step with the likelihood left to the forward's own softmax launch (VARGP_DEFER_SOFTMAX=0, read per step): the
    tile kernel's likelihood alone against the kernel VARGP.loss uses, everything else equal."""
    res = []
    for defer in ('1', '0'):
        monkeypatch.setenv('VARGP_DEFER_SOFTMAX', defer)
        tr, sc, grads, _ = _trainer_step(shape, map_est)
        assert tr._prog.plan()['defer_softmax'] == (defer == '1')
        res.append((sc, grads))
    (sc_d, g_d), (sc_u, g_u) = res
    for k in SCALARS:
        print(shape, k, sc_d[k], sc_u[k])
        np.testing.assert_allclose(sc_d[k], sc_u[k], rtol=1e-5, err_msg=k)
    for k in g_u:
        e = rel_l2(g_d[k], g_u[k])
        print(shape, 'grad', k, '%.2e' % e)
        assert e < 1e-5, k


@pytest.mark.parametrize('shape,map_est,want', NATIVE, ids=_ids(NATIVE))
def test_native_noise_step_matches_fp64_oracle(shape, map_est, want):
    """The trainer's default: noise drawn by the forward into the workspace, read there by the deferred likelihood (float4).  The
    oracle gets the draws as the program's workspace views hold them after the step."""
    tr, sc, grads, nz = _trainer_step(shape, map_est, native=True)
    plan = tr._prog.plan()
    print(shape, 'plan:', plan)
    assert tr.native_noise and plan['native'] and plan['defer_softmax']
    _assert_plan(plan, want, shape)
    assert torch.isfinite(nz['eps_f']).all() and 0.9 < nz['eps_f'].std().item() < 1.1      # (draws, not stale memory)
    _check_against_oracle(f'{shape} native', sc, grads, *_oracles(shape, map_est, nz))


@pytest.mark.parametrize('shape,map_est,want', GRAPH, ids=_ids(GRAPH))
def test_graph_replay_matches_fp64_oracle(shape, map_est, want):
    tr, sc, grads, _ = _trainer_step(shape, map_est, graph=True)
    _assert_plan(tr._prog.plan(), want, shape)
    _check_against_oracle(f'{shape} graph', sc, grads, *_oracle(shape, map_est))


def test_loss_route_native_noise_vs_fp64():
    """VARGP.loss without injected noise: the program's own draws on the route that does not defer the likelihood."""
    from gpu_common import build_gp, grads_of
    shape = LOSS_NATIVE
    S, F_, C, M, D, B = shape
    params, prev, x, y, _ = _problem(shape)
    gp = build_gp(params, prev, S, F_)
    kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
    (BETA * kl_h + kl_u + 7.0 * nll).backward()
    torch.cuda.synchronize()
    prog = next(iter(gp._t0_progs.values()))
    plan = prog.plan()
    assert plan['native'] and not plan['defer_softmax'] and plan['fwd_softmax16'], plan
    nz = dict(eps_theta=prog.eps_theta().detach().clone().cpu(), eps_f=prog.eps_f().detach().clone().cpu())
    sc = dict(kl_hypers=kl_h.item(), kl_u=kl_u.item(), nll=nll.item())
    grads = {k: g.detach().cpu() for k, g in grads_of(gp).items()}
    _check_against_oracle(f'{shape} loss, native', sc, grads, *_oracles(shape, False, nz))
