"""The parity rule of the randomised sweeps (tests/test_hip_random_sweep.py states it in full), shared by every module that
applies it: per case and per class of quantities (the three ELBO scalars by relative error, the five gradients by relative
L2 norm),

    max_q err_q(HIP, fp64 oracle)  <=  tolerance  +  2 x max_q err_q(fp32 oracle, fp64 oracle).

A case is a dict(S, F, C, M, n_prev, D, B, nomean, seed).  `composed=True` runs VARGP.loss with fused_first_task and fused_tasks
cleared (the op-by-op autograd route of vargp_amd/ops.py) and asserts that no native program was created on the model."""
import torch

from oracle import vargp_oracle as orc
from helpers import REL_L2_GRAD, RTOL_SCALAR, rel_l2, to_dev

DEV = 'cuda:0'
COST_CAP = 2.5e9          # host-oracle flop proxy per case (see _cost): keeps a sweep's fp64 oracle time to tens of seconds


def _dbl(t):
    if isinstance(t, torch.Tensor):
        return t.double() if t.is_floating_point() else t
    if isinstance(t, dict):
        return {k: _dbl(v) for k, v in t.items()}
    if isinstance(t, (list, tuple)):
        return type(t)(_dbl(v) for v in t)
    return t


def _cost(S, C, M, n_prev, D, B):
    Mt = M * (n_prev + 1)
    return S * C * (Mt * Mt * (D + B + Mt) + Mt * B * D)


def oracle_pair(c):
    """-> (problem, fp32 oracle (scalars, grads), fp64 oracle (scalars, grads)) of one case."""
    kind = 'wtoy' if c['D'] == 2 else 'gauss'
    prob = orc.make_problem(c['S'], c['F'], c['C'], c['M'], c['D'], c['B'], n_prev=c['n_prev'], seed=c['seed'], kind=kind)
    params, prev, x, y, nz = prob
    kw = dict(beta=2.0, n_total=7 * c['B'], ep_var_mean=not c['nomean'])
    # The fp32 oracle runs on ONE host thread: the host BLAS rounds differently for every thread count, and on the
    # ill-conditioned cases that moves the fp32 error -- and with it the bound -- by more than an order of magnitude
    # (seed 317, Mt = 600 in D = 4: nll 1.2e-3 on one thread, 3e-5 on four).  The bound then does not depend on the host.
    n_threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        r32 = orc.elbo_step(params, prev, x, y, nz, **kw)
    finally:
        torch.set_num_threads(n_threads)
    r64 = orc.elbo_step(_dbl(params), _dbl(prev), _dbl(x), y, _dbl(nz), **kw)
    return prob, r32, r64


def _hip(c, prob, composed=False):
    from gpu_common import build_gp, grads_of
    from vargp_amd import noise
    params, prev, x, y, nz = prob
    gp = build_gp(params, prev, c['S'], c['F'], ep_var_mean=not c['nomean'])
    if composed:
        gp.fused_first_task = gp.fused_tasks = False
    on_block = bool(gp._use_block_program(c['B']))
    with noise.inject(**to_dev(nz, DEV)):
        kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
        (2.0 * kl_h + kl_u + 7.0 * nll).backward()
    if composed:
        progs = (gp._t0_progs, gp._t0_spares, gp._tn_progs, gp._tn_spares)
        assert not on_block and not any(progs), f'composed route created a native program: {progs}'
    sc = dict(kl_hypers=float(kl_h), kl_u=float(kl_u), nll=float(nll))
    gr = {k: v.detach().cpu().double() for k, v in grads_of(gp).items()}
    gp.release_programs()
    return sc, gr, on_block


def _sweep(cases, label, composed=False):
    from vargp_amd import ops
    ops.set_cholesky_error_mode('raise')
    rows, bad = [], []
    for c in cases:
        prob, (s32, g32), (s64, g64) = oracle_pair(c)
        sc, gr, on_block = _hip(c, prob, composed=composed)
        worst = (0.0, None, 0.0, 0.0)                      # (err / bound, quantity, err, bound)
        strict_bad = []                                    # quantities outside the per-quantity form of the rule
        e_sc = {k: (abs(v - s64[k].item()) / abs(s64[k].item()), abs(s32[k].item() - s64[k].item()) / abs(s64[k].item()))
                for k, v in sc.items() if s64[k].item() != 0.0}
        e_gr = {'grad ' + k: (rel_l2(g, g64[k]), rel_l2(g32[k].double(), g64[k])) for k, g in gr.items()}
        for errs, tol in ((e_sc, RTOL_SCALAR), (e_gr, REL_L2_GRAD)):
            bound = tol + 2.0 * max(e32 for _, e32 in errs.values())
            for k, (e_hip, e_32) in errs.items():
                if e_hip / bound > worst[0]:
                    worst = (e_hip / bound, k, e_hip, bound)
                if e_hip > max(tol, 2.0 * e_32):
                    strict_bad.append((k, e_hip, max(tol, 2.0 * e_32)))
        tag = 'S{S} F{F} C{C} M{M} t{n_prev} D{D} B{B} nomean={nm} seed={seed}'.format(nm=int(c['nomean']), **c)
        rows.append((worst, tag, on_block, strict_bad))
        print(f'[{label}] {tag} block={int(on_block)}: worst {worst[1]} err {worst[2]:.2e} (bound {worst[3]:.2e})'
              + (f'   strict: {[(k, "%.2e" % e, "%.2e" % bd) for k, e, bd in strict_bad]}' if strict_bad else ''), flush=True)
        if worst[0] > 1.0:
            bad.append((tag, worst))
    w = max(rows, key=lambda r: r[0][0])
    print(f'[{label}] {len(rows)} cases, {sum(r[2] for r in rows)} on the block program; worst case: {w[1]}: {w[0][1]} err '
          f'{w[0][2]:.2e} against the bound {w[0][3]:.2e} ({w[0][0]:.2f} of it); loosest bound used: '
          f'{max(r[0][3] for r in rows):.2e}; per-quantity form of the rule: {sum(not r[3] for r in rows)} of {len(rows)} cases pass')
    assert not bad, f'{len(bad)} of {len(rows)} {label} cases outside tolerance + 2 x fp32-oracle error of the class: {bad}'
    return rows
