"""GPU: the first-task step with the small-column product QP[:, :NR] = T [m | L_S | L_u] folded into t0_fwd_fused_kernel
(T0Plan::fold_small, csrc/elbo_t0.hip): G = T L_S and a = T m recomputed by every tile workgroup, G2 = T L_u and the KL of q(u)
by role workgroups on the CUs the tiles leave free.

Shapes (D = 32 throughout): M in {36, 100, 104} -- two 32-row blocks, a 4-row last block, the padded limit; B in {64, 132, 512} --
one tile, a ragged last tile with B % 4 == 0, eight tiles; (S, C) in {(1, 2), (3, 3), (3, 10)} -- (3, 3) and (3, 10) put more than
eight matrices on the XCD map and give role workgroups two matrices.  B = 512 and (3, 10) at M = 100 only.

Per case: QP[:, :NR] = (a, G, G2), the moments mu / var, the three loss terms and every gradient
  * against fp64 (oracle/vargp_oracle.py in double precision; a, G, G2 as triangular solves against the fp64 factors),
  * folded against unfolded (VARGP_T0_FOLD_SMALL=0, read once per process: the unfolded results come from ONE child process
    that runs every case),
  * and one captured-graph replay against the eager step.

Tolerances come from neither path under test alone: a quantity's error against fp64 is measured on the UNFOLDED plan, and the
folded plan is allowed twice that, floored at what tests/test_hip_t0_program.py holds the quantity to -- helpers.RTOL_SCALAR for
the loss terms, helpers.REL_L2_GRAD for the gradients.  That file does not check QP, mu and var; their floor is RTOL_SCALAR as a
relative L2 error: kl_u and nll are smooth functions of exactly these arrays and are held to it.  (The folded product sums the
same fp32 products in another order, not in lower precision.)  Folded against unfolded: three times the same bound, the sum of
the two distances to fp64.  Graph against eager: 1e-5, as test_hip_train.test_graph_step_equals_eager_step.

Measured on MI355X over the 17 cases, largest error against fp64, folded / unfolded: a 9.2e-7 / 9.1e-7, G 8.8e-7 / 8.8e-7, G2
8.7e-7 / 8.8e-7, mu 4.3e-6 / 4.3e-6, var 7.4e-7 / 7.4e-7, kl_u 1.6e-7 / 3.7e-7, nll 1.2e-7 / 1.2e-7, g_z 1.3e-6 / 1.3e-6, g_u_mean
1.3e-6 / 1.3e-6, g_u_tril_vec 1.2e-6 / 1.2e-6, g_log_mean 4.0e-7 / 3.0e-7, g_log_logvar 4.2e-7 / 5.2e-7.  Largest ratio folded /
unfolded in one case: arrays and the z, u gradients <= 1.04; the scalars and hyper-gradients, whose errors sit at 1e-8 .. 5e-7 (a
few fp32 roundings), up to 6.0 (kl_u), 4.5 (nll), 6.0 (g_log_logvar), 2.8 (g_log_mean) -- every one of them below its floor by a
factor of 200 or more.  Folded against unfolded: <= 7.8e-7 (g_z) everywhere."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import rel_l2, to_dev, RTOL_SCALAR, REL_L2_GRAD

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEED = 31
D, F_ = 32, 2
HERE = os.path.dirname(os.path.abspath(__file__))

# (S, F, C, M, D, B)
CASES = [(S, F_, C, M, D, B) for M in (36, 100, 104) for B in (64, 132, 512) for (S, C) in ((1, 2), (3, 3), (3, 10))
         if M == 100 or (B != 512 and (S, C) != (3, 10))]
IDS = [str(c) for c in CASES]
SCALARS = ('kl_hypers', 'kl_u', 'nll')
ARRAYS = ('a', 'G', 'G2', 'mu', 'var')


def _ws_qp(S, F, C, M, D_, B):
    """Float offset of QP in a first-task workspace, NR and LD (elbo_t0.hip: carve_t0)."""
    r = lambda n: (n + 63) // 64 * 64
    SC, MM, Dp = S * C, M * M, (D_ + 3) // 4 * 4
    NR = (4 + 2 * M + 3) // 4 * 4
    LD = (NR + B + 3) // 4 * 4
    off = 0
    for n in (S * (D_ + 1), S * (D_ + 1), S * F * C * B, S * Dp, S, SC, 8, SC * M, S * B, S * B * D_, C * MM, (SC + C) * MM,
              (SC + C) * MM, (SC + C) * MM, SC * M * LD):
        off += r(n)
    return off, NR, LD


def _run(case):
    """One step of the program on `case` under this process's plan -> dict of CPU tensors / floats."""
    from vargp_amd import noise
    from gpu_common import build_gp, grads_of
    S, F, C, M, D_, B = case
    params, prev, x, y, nz = orc.make_problem(S, F, C, M, D_, B, n_prev=0, seed=SEED)
    gp = build_gp(params, prev, S, F)
    with noise.inject(**to_dev(nz, DEV)):
        kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
        torch.cuda.synchronize()
        prog = next(iter(gp._t0_progs.values()))
        off, NR, LD = _ws_qp(*case)
        qp = prog.ws[off: off + S * C * M * LD].view(S, C, M, LD)[..., :NR].detach().cpu().clone()
        mu, var = (t.detach().cpu().clone() for t in prog.lik_buffers()[:2])
        (2.0 * kl_h + kl_u + 7.0 * nll).backward()
    out = dict(kl_hypers=kl_h.item(), kl_u=kl_u.item(), nll=nll.item(), mu=mu, var=var,
               a=qp[..., 0], G=qp[..., 4:4 + M], G2=qp[..., 4 + M:4 + 2 * M], small_rest=qp[..., 1:4])
    out.update({'g_' + k: g.detach().cpu() for k, g in grads_of(gp).items()})
    return out


def _dump_unfolded(path):
    """(child process, VARGP_T0_FOLD_SMALL=0) every case under the unfolded plan -> path"""
    assert os.environ.get('VARGP_T0_FOLD_SMALL') == '0'
    torch.save({c: _run(c) for c in CASES}, path)


def _fp64(case):
    S, F, C, M, D_, B = case
    params, prev, x, y, nz = orc.make_problem(S, F, C, M, D_, B, n_prev=0, seed=SEED)
    dbl = lambda d: {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}
    p64, n64, x64 = dbl(params), dbl(nz), x.double()
    sc, og = orc.elbo_step(p64, prev, x64, y, n64, beta=2.0, n_total=7 * B)
    mu, var, _ = orc.forward(p64, prev, x64, n64)
    theta = orc.sample_hypers(p64['log_mean'], p64['log_logvar'], n64['eps_theta'])
    Lz = orc.chol(orc.rbf_gram(theta, p64['z']))                          # (S, C, M, M)
    Lu = orc.vec2tril(p64['u_tril_vec'], M)
    LS = orc.chol(orc.llt(Lu))
    solve = lambda rhs: torch.linalg.solve_triangular(Lz, rhs.unsqueeze(0).expand(S, *rhs.shape), upper=False)
    out = dict(kl_hypers=sc['kl_hypers'].item(), kl_u=sc['kl_u'].item(), nll=sc['nll'].item(), mu=mu, var=var,
               a=solve(p64['u_mean'].reshape(C, M, 1)).squeeze(-1), G=solve(LS), G2=solve(Lu))
    out.update({'g_' + k: g for k, g in og.items()})
    return out


_CACHE = {}


def _unfolded():
    if 'unfolded' not in _CACHE:
        assert os.environ.get('VARGP_T0_FOLD_SMALL', '1') == '1', 'this process must run the folded plan'
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'unfolded.pt')
            code = 'import sys; sys.path[:0] = [%r, %r]; import test_hip_fold_small as t; t._dump_unfolded(%r)' % (
                os.path.dirname(HERE), HERE, path)
            r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, VARGP_T0_FOLD_SMALL='0'), capture_output=True,
                               text=True, timeout=600)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            _CACHE['unfolded'] = torch.load(path, weights_only=False)
    return _CACHE['unfolded']


def _case(case):
    """(folded, unfolded, fp64) results of `case`: computed once, shared by the tests, never modified."""
    if case not in _CACHE:
        _CACHE[case] = (_run(case), _unfolded()[case], _fp64(case))
    return _CACHE[case]


def _err(v, ref):
    return abs(v - ref) / abs(ref) if isinstance(v, float) else rel_l2(v, ref)


def _quantities(res):
    return [(k, RTOL_SCALAR) for k in SCALARS] + [(k, RTOL_SCALAR) for k in ARRAYS] + \
           [(k, REL_L2_GRAD) for k in sorted(res) if k.startswith('g_')]


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_folded_plan_matches_fp64(case):
    """Every quantity of the folded plan within twice the unfolded plan's error against fp64 (floored: module docstring)."""
    fold, unf, ref = _case(case)
    bad = []
    for k, floor in _quantities(fold):
        e_f, e_u = _err(fold[k], ref[k]), _err(unf[k], ref[k])
        print(case, k, 'folded %.3e unfolded %.3e ratio %.2f' % (e_f, e_u, e_f / max(e_u, 1e-30)))
        if not e_f <= max(2.0 * e_u, floor):
            bad.append((k, e_f, e_u))
    assert not bad, bad
    # columns 1 .. 3 of QP: zero on both plans (T times RK's zero columns)
    assert not fold['small_rest'].any() and torch.equal(fold['G'], fold['G'].tril()) and torch.equal(fold['G2'], fold['G2'].tril())


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_folded_plan_matches_unfolded_plan(case):
    """Folded against unfolded through the tuning switch: within the sum of the two distances to fp64 allowed above."""
    fold, unf, ref = _case(case)
    bad = []
    for k, floor in _quantities(fold):
        e_fu, e_u = _err(fold[k], unf[k]), _err(unf[k], ref[k])
        print(case, k, 'folded vs unfolded %.3e (unfolded vs fp64 %.3e)' % (e_fu, e_u))
        if not e_fu <= 3.0 * max(e_u, floor):
            bad.append((k, e_fu, e_u))
    assert not bad, bad


@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_graph_replay_equals_eager_step(case):
    """One replay of the captured step against one eager step from the same state and noise."""
    from vargp_amd import noise, ops
    from vargp_amd.train import ElboTrainer
    from gpu_common import build_gp
    S, F, C, M, D_, B = case
    params, prev, x, y, nz = orc.make_problem(S, F, C, M, D_, B, n_prev=0, seed=SEED)
    xd, yd = x.to(DEV), y.to(DEV)
    ops.set_cholesky_error_mode('defer')
    ops.reset_linalg_errors()
    try:
        results = []
        for mode in ('eager', 'graph'):
            gp = build_gp(params, prev, S, F)
            tr = ElboTrainer(gp, lr=1e-3, beta=10.0, n_total=12000)
            with noise.inject(**to_dev(nz, DEV)):
                if mode == 'graph':
                    tr.capture(xd, yd, warmup=2)
                for _ in range(1):
                    out = [o.item() for o in (tr.step_graph() if mode == 'graph' else tr.step(xd, yd))]
            torch.cuda.synchronize()
            results.append(({k: v.detach().cpu().clone() for k, v in gp.state_dict().items()}, np.array(out)))
        (sd_e, out_e), (sd_g, out_g) = results
        np.testing.assert_allclose(out_g, out_e, rtol=1e-5)
        for k in sd_e:
            assert rel_l2(sd_g[k], sd_e[k]) < 1e-5, k
        assert ops.linalg_error_count() == 0
    finally:
        ops.set_cholesky_error_mode('raise')
