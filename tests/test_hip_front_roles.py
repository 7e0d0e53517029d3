"""GPU: the first-task step whose single-use outputs P, W (t0_fwd_fused_kernel) and W_uf (t0_bwd_mid_kernel) leave their kernels
through write-through stores (common.h: store_once), and the S_u / L_S it factorises on the way.

Shapes: M in {68, 100} is the blocked-chain range 64 < n <= 100 with a ragged last 16-block, M = 64 the other chain path;
B in {64, 72, 132} a full 64-column tile and ragged last tiles with B % 4 == 0; S in {1, 3}, C in {1, 3}.  D = 32 is the
direct distance form: it runs the tile kernels (every streamed output) but neither the front launch nor the merged
factorisation launch, which need D >= 256 (T0Plan::split_kuu) -- so the same shapes also run at D = 256, the smallest D with
the eight-launch step of the benchmark.  Tolerances are the ones the existing tests hold the same quantities to:
helpers.RTOL_SCALAR / REL_L2_GRAD (test_hip_t0_program), 1e-5 on a Cholesky factor (test_hip_ops.test_chol_inv_fwd_bwd),
1e-5 graph against eager (test_hip_train.test_graph_step_equals_eager_step)."""
import numpy as np
import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import rel_l2, to_dev, RTOL_SCALAR, REL_L2_GRAD

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
JITTER = 1e-4
SEED = 31

# (S, F, C, M, D, B): every value of M, B, S and C named above occurs with D = 32 and with D = 256
_SMCB = [(3, 3, 100, 132), (1, 3, 100, 72), (3, 1, 68, 72), (1, 1, 68, 64), (3, 3, 68, 132), (3, 3, 64, 72)]
SHAPES = [(S, 2, C, M, D, B) for D in (32, 256) for (S, C, M, B) in _SMCB]
FRONT_SHAPES = [s for s in SHAPES if s[4] == 256 and s[3] > 64]      # the merged launch's blocked chains build S_u themselves


def _ws_offsets(S, F_, C, M, D, B):
    """Float offsets of Lu, KS = [K_uu | S_u] and LL = [L_z | L_S] in a first-task workspace (elbo_t0.hip: carve_t0)."""
    r = lambda n: (n + 63) // 64 * 64
    SC, MM, Dp = S * C, M * M, (D + 3) // 4 * 4
    off = 0
    for n in (S * (D + 1), S * (D + 1), S * F_ * C * B, S * Dp, S, SC, 8, SC * M, S * B, S * B * D):
        off += r(n)
    lu = off
    ks = lu + r(C * MM)
    ll = ks + r((SC + C) * MM)
    return lu, ks, ll


def _su_ls(gp, shape):
    """(S_u, L_S), each (C, M, M), as the last forward of `gp` left them in its program's workspace.  Every plan writes L_u in
    front of them: it must be where _ws_offsets says, or the layout has changed and _ws_offsets with it."""
    S, F_, C, M, D, B = shape
    prog = next(iter(gp._t0_progs.values()))
    lu, ks, ll = _ws_offsets(*shape)
    MM = M * M
    lu_ws = prog.ws[lu: lu + C * MM].view(C, M, M).detach().cpu()
    assert rel_l2(lu_ws, orc.vec2tril(gp.u_tril_vec.detach().cpu().double(), M)) < 1e-6, \
        'L_u is not at its offset: carve_t0 (csrc/elbo_t0.hip) no longer matches _ws_offsets'
    su = prog.ws[ks + S * C * MM: ks + (S * C + C) * MM].view(C, M, M)
    ls = prog.ws[ll + S * C * MM: ll + (S * C + C) * MM].view(C, M, M)
    return su.detach().cpu().clone(), ls.detach().cpu().clone()


_CACHE = {}


def _case(shape):
    """Problem, oracle step and the program's results of `shape`: computed once, shared by the tests, never modified."""
    if shape not in _CACHE:
        from vargp_amd import noise
        from gpu_common import build_gp, grads_of
        S, F_, C, M, D, B = shape
        params, prev, x, y, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=0, seed=SEED)
        gp = build_gp(params, prev, S, F_)
        with noise.inject(**to_dev(nz, DEV)):
            kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
            torch.cuda.synchronize()
            su, ls = _su_ls(gp, shape)
            (2.0 * kl_h + kl_u + 7.0 * nll).backward()
        sc, og = orc.elbo_step(params, prev, x, y, nz, beta=2.0, n_total=7 * B)
        _CACHE[shape] = dict(params=params, scalars=dict(kl_hypers=kl_h.item(), kl_u=kl_u.item(), nll=nll.item()),
                             grads={k: g.cpu() for k, g in grads_of(gp).items()}, sc=sc, og=og, su=su, ls=ls)
    return _CACHE[shape]


def _check_step(shape):
    r = _case(shape)
    for k, v in r['scalars'].items():
        print(shape, k, v, r['sc'][k].item())
        np.testing.assert_allclose(v, r['sc'][k].item(), rtol=RTOL_SCALAR, err_msg=k)
    for k, g in r['grads'].items():
        print(shape, k, rel_l2(g, r['og'][k]))
        assert rel_l2(g, r['og'][k]) < REL_L2_GRAD, k


@pytest.mark.parametrize('shape', SHAPES, ids=[str(s) for s in SHAPES])
def test_step_matches_fp64_oracle(shape):
    """Loss terms and every gradient of one step: K_uf, P, W, W_uf and P_uf end to end."""
    _check_step(shape)


@pytest.mark.parametrize('shape', SHAPES, ids=[str(s) for s in SHAPES])
def test_su_and_ls_match_fp64(shape):
    """L_S = chol(S_u + jitter I) read back from the workspace, and S_u = L_u L_u^T where the plan leaves it there: the blocked
    chains of the merged launch (T0Plan::su_in_chain: D >= 256, 64 < M <= 100) build S_u in LDS and write only its factor."""
    S, F_, C, M, D, B = shape
    r = _case(shape)
    lu64 = orc.vec2tril(r['params']['u_tril_vec'].double(), M)
    su64 = orc.llt(lu64)
    ls64 = orc.chol(su64, JITTER)
    e_ls = rel_l2(r['ls'].tril(), ls64)
    print(shape, 'L_S', e_ls)
    assert e_ls < 1e-5
    if shape not in FRONT_SHAPES:
        e_su = rel_l2(r['su'], su64)
        print(shape, 'S_u', e_su)
        assert e_su < 1e-5
        assert torch.equal(r['su'], r['su'].transpose(-1, -2))


@pytest.mark.parametrize('shape', [FRONT_SHAPES[0], SHAPES[0]], ids=str)
def test_ten_graph_replays_equal_ten_eager_steps(shape):
    """A consumer that read a streamed line before it had landed would show here: ten replays of the captured step against ten
    eager steps from the same seeded state."""
    from vargp_amd import noise, ops
    from vargp_amd.train import ElboTrainer
    from gpu_common import build_gp
    S, F_, C, M, D, B = shape
    params, prev, x, y, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=0, seed=SEED)
    xd, yd = x.to(DEV), y.to(DEV)
    ops.set_cholesky_error_mode('defer')
    ops.reset_linalg_errors()
    try:
        results = []
        for mode in ('eager', 'graph'):
            gp = build_gp(params, prev, S, F_)
            tr = ElboTrainer(gp, lr=1e-3, beta=10.0, n_total=12000)
            outs = []
            with noise.inject(**to_dev(nz, DEV)):
                if mode == 'graph':
                    tr.capture(xd, yd, warmup=2)
                for _ in range(10):
                    out = tr.step_graph() if mode == 'graph' else tr.step(xd, yd)
                    outs.append([o.item() for o in out])
            torch.cuda.synchronize()
            results.append(({k: v.detach().cpu().clone() for k, v in gp.state_dict().items()}, np.array(outs)))
        (sd_e, out_e), (sd_g, out_g) = results
        np.testing.assert_allclose(out_g, out_e, rtol=1e-5)
        for k in sd_e:
            assert rel_l2(sd_g[k], sd_e[k]) < 1e-5, k
        assert ops.linalg_error_count() == 0
    finally:
        ops.set_cholesky_error_mode('raise')


def test_unmerged_plan_still_builds_su_in_its_chain():
    """S C + C chains above half the CU count (132 on 256 CUs): the launches are taken apart (T0Plan::unmerge: from a third of the
    CU count on) and the chain workgroup builds S_u itself (in LDS: only its factor reaches the workspace)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    C = 3
    S = (cus // 2) // C + 1
    assert S * C + C > cus // 2 and S * C + C >= cus // 3 + 1          # t0_plan's rule for `unmerge` (csrc/elbo_t0.hip)
    shape = (S, 1, C, 68, 256, 64)
    _check_step(shape)
    r = _case(shape)
    su64 = orc.llt(orc.vec2tril(r['params']['u_tril_vec'].double(), shape[3]))
    e_ls = rel_l2(r['ls'].tril(), orc.chol(su64, JITTER))
    print(shape, 'L_S', e_ls)
    assert e_ls < 1e-5
