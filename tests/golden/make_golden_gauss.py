"""Golden vectors of VAR-GP regression (GaussianLikelihood, var_gp/likelihoods.py:66-110) from the REFERENCE, imported
read-only from /root/reference, with the hyper-parameter noise (and eps_u) injected exactly as make_golden.py does.
Run in the build container only:

    python tests/golden/make_golden_gauss.py [names...]

Writes tests/golden/gauss_*.npz and retrain_gauss_*.npz (data only).  Regression targets and per-output observation
log-variances are closed-form functions of the seed (`targets`, `obs_log_var` below; tests/test_hip_gauss.py restates them
for the full-size case, whose inputs are regenerated rather than stored).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import ROOT, injected, npify, orc, ref_kernels, ref_lik, ref_vargp, _tdn, _tdm  # noqa: E402,F401

assert ROOT in sys.path


def targets(x, C, seed, bcast=False):
    """Smooth regression targets of the inputs: y[c, b] = sin(w_c . x_b + c) + 0.1 noise  ((B,) for bcast)."""
    D = x.shape[1]
    w = orc.hash_normal((C, D), seed + 201) * (2.0 / np.sqrt(max(D * 0.25, 1.0)))
    f = torch.sin(x.double() @ w.mT + torch.arange(C, dtype=torch.float64)).mT           # (C, B)
    y = f + 0.1 * orc.hash_normal(tuple(f.shape), seed + 203)
    return (y[0] if bcast else y).float()


def obs_log_var(C):
    return torch.linspace(-2.5, -0.5, C, dtype=torch.float64).float()


def build_ref(params, prev, S, ep_var_mean=True, olv=None):
    D = params['z'].shape[-1]
    kern = ref_kernels.RBFKernel(D, prior_log_mean=params['prior_log_mean'].clone(),
                                 prior_log_logvar=params['prior_log_logvar'].clone())
    kern.log_mean.data.copy_(params['log_mean'])
    kern.log_logvar.data.copy_(params['log_logvar'])
    C = params['z'].shape[0]
    lik = ref_lik.GaussianLikelihood(C)
    lik.obs_log_var.data.copy_(olv if olv is not None else obs_log_var(C))
    gp = ref_vargp.VARGP(params['z'].clone(), kern, lik, n_var_samples=S, ep_var_mean=ep_var_mean,
                         prev_params=[{k: v.clone() for k, v in p.items()} for p in prev])
    gp.u_mean.data.copy_(params['u_mean'])
    gp.u_tril_vec.data.copy_(params['u_tril_vec'])
    return gp


def gauss_case(name, S, C, M, D, B, n_prev, seed, kind, beta, n_total, bcast=False, ep_var_mean=True, store_inputs=True,
               prev_from_state_dict=False):
    params, prev, x, _, noise = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=seed, kind=kind)
    noise = {k: v for k, v in noise.items() if k != 'eps_f'}          # the Gaussian likelihood draws no noise
    y = targets(x, C, seed, bcast)
    if prev_from_state_dict:
        # task 1 of a continual regression run: the earlier task is the state_dict() of a task-0 GaussianLikelihood model (its
        # kernel.* and likelihood.obs_log_var keys are carried along and ignored, reference vargp.py:17-20)
        p0 = dict(params, **prev[0])
        gp0 = build_ref(p0, [], S, olv=obs_log_var(C) - 0.3)
        prev = [{k: v.detach().clone() for k, v in gp0.state_dict().items()}]
    gp = build_ref(params, prev, S, ep_var_mean)
    with injected(noise):
        kl_h, kl_u, nll = gp.loss(x, y)
        total = beta * kl_h + kl_u + (n_total / B) * nll
        gp.zero_grad()
        total.backward()
    grads = dict(z=gp.z.grad, u_mean=gp.u_mean.grad, u_tril_vec=gp.u_tril_vec.grad, log_mean=gp.kernel.log_mean.grad,
                 log_logvar=gp.kernel.log_logvar.grad, obs_log_var=gp.likelihood.obs_log_var.grad)
    with injected(noise), torch.no_grad():
        pmu, pvar = gp(x)
    with injected(noise), torch.no_grad():
        pred = gp.predict(x)
    assert torch.equal(pred, pmu)
    out = dict(meta=np.array([S, 1, C, M, D, B, n_prev, seed], dtype=np.int64), kind=np.array(kind),
               beta=np.float64(beta), n_total=np.float64(n_total), ep_var_mean=np.int64(ep_var_mean), bcast=np.int64(bcast),
               kl_hypers=kl_h.item(), kl_u=kl_u.item(), nll=nll.item(), total=total.item(),
               pred_mu=pmu.numpy(), pred_var=pvar.numpy(), p_obs_log_var=obs_log_var(C).numpy())
    if store_inputs:
        out.update(npify(grads, 'grad_'))
        out.update(npify(params, 'p_'))
        for i, p in enumerate(prev):
            out.update(npify({k: p[k] for k in ('z', 'u_mean', 'u_tril_vec')}, f'prev{i}_'))
        if prev_from_state_dict:
            out.update(npify({k: v for k, v in prev[0].items() if k not in ('z', 'u_mean', 'u_tril_vec')}, 'prev0sd_'))
        out.update(npify(noise, 'n_'))
        out.update(x=x.numpy(), y=y.numpy())
    else:   # full-size case: inputs are regenerated from the seed; compact checks only
        for k, g in grads.items():
            out[f'gradnorm_{k}'] = g.double().norm().item()
        out['grad_log_mean'] = grads['log_mean'].numpy()
        out['grad_obs_log_var'] = grads['obs_log_var'].numpy()
        out['grad_u_mean'] = grads['u_mean'].numpy()
        out['grad_z_head'] = grads['z'][:, :4, :].numpy()
        out['pred_mu'], out['pred_var'] = out['pred_mu'][..., :64], out['pred_var'][..., :64]
    np.savez_compressed(os.path.join(HERE, f'{name}.npz'), **out)
    print(f'{name}: kl_h={kl_h.item():.6f} kl_u={kl_u.item():.6f} nll={nll.item():.6f}')


def retrain_gauss_case(name, S, C, M, D, B, n_prev, seed, kind, beta, n_total):
    """VARGPRetrain (var_gp/vargp_retrain.py) with a GaussianLikelihood: loss triple and the gradients of the current and the
    re-optimised earlier-task parameters (the two MultivariateNormal.sample() draws injected by shape)."""
    import var_gp.vargp_retrain as ref_rt
    params, prev, x, _, noise = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=seed, kind=kind)
    y = targets(x, C, seed)
    Mt = (n_prev + 1) * M
    noise = dict(eps_theta=noise['eps_theta'], eps_u_leq=orc.hash_normal((S, S, C, Mt), seed + 51).float(),
                 eps_u_tilde=orc.hash_normal((S, S, S, C, Mt - M), seed + 53).float())
    kern = ref_kernels.RBFKernel(D, prior_log_mean=params['prior_log_mean'].clone(),
                                 prior_log_logvar=params['prior_log_logvar'].clone())
    kern.log_mean.data.copy_(params['log_mean'])
    kern.log_logvar.data.copy_(params['log_logvar'])
    lik = ref_lik.GaussianLikelihood(C)
    lik.obs_log_var.data.copy_(obs_log_var(C))
    gp = ref_rt.VARGPRetrain(params['z'].clone(), kern, lik, n_var_samples=S,
                             prev_params=[{k: v.clone() for k, v in p.items()} for p in prev])
    gp.u_mean.data.copy_(params['u_mean'])
    gp.u_tril_vec.data.copy_(params['u_tril_vec'])
    o_n, o_m = _tdn._standard_normal, _tdm._standard_normal

    def std_normal_mvn(shape, dtype, device):
        for k in ('eps_u_leq', 'eps_u_tilde'):
            if tuple(shape) == tuple(noise[k].shape):
                return noise[k].to(dtype)
        raise AssertionError(shape)

    _tdn._standard_normal = lambda shape, dtype, device: noise['eps_theta'].to(dtype)
    _tdm._standard_normal = std_normal_mvn
    try:
        kl_h, kl_u, nll = gp.loss(x, y)
        total = beta * kl_h + kl_u + (n_total / B) * nll
        gp.zero_grad()
        total.backward()
    finally:
        _tdn._standard_normal, _tdm._standard_normal = o_n, o_m
    out = dict(meta=np.array([S, 1, C, M, D, B, n_prev, seed], dtype=np.int64), kind=np.array(kind),
               beta=np.float64(beta), n_total=np.float64(n_total),
               kl_hypers=kl_h.item(), kl_u=kl_u.item(), nll=nll.item(), total=total.item(),
               p_obs_log_var=obs_log_var(C).numpy())
    grads = dict(z=gp.z.grad, u_mean=gp.u_mean.grad, u_tril_vec=gp.u_tril_vec.grad, log_mean=gp.kernel.log_mean.grad,
                 log_logvar=gp.kernel.log_logvar.grad, obs_log_var=gp.likelihood.obs_log_var.grad)
    out.update(npify(grads, 'grad_'))
    for i, pd in enumerate(gp.retrain_params):
        out.update({f'grad_retrain{i}_{k}': pd[k].grad.detach().numpy() for k in ('z', 'u_mean', 'u_tril_vec')})
    out.update(npify(params, 'p_'))
    for i, p in enumerate(prev):
        out.update(npify(p, f'prev{i}_'))
    out.update(npify(noise, 'n_'))
    out.update(x=x.numpy(), y=y.numpy())
    np.savez_compressed(os.path.join(HERE, f'{name}.npz'), **out)
    print(f'{name}: kl_h={kl_h.item():.6f} kl_u={kl_u.item():.6f} nll={nll.item():.6f}')


if __name__ == '__main__':
    only = set(sys.argv[1:])
    cases = [
        # toy size (S3 C4 M20 D2 B100), first task: targets per output, and one target row broadcast over the outputs
        ('gauss_t0', dict(S=3, C=4, M=20, D=2, B=100, n_prev=0, seed=301, kind='wtoy', beta=1.0, n_total=100)),
        ('gauss_t0_bcast', dict(S=3, C=4, M=20, D=2, B=100, n_prev=0, seed=302, kind='wtoy', beta=1.0, n_total=100,
                                bcast=True)),
        # task 1, the earlier task taken from a task-0 model's state_dict(); and the ep_var_mean=False ablation
        ('gauss_t1', dict(S=3, C=4, M=20, D=2, B=100, n_prev=1, seed=303, kind='wtoy', beta=1.0, n_total=100,
                          prev_from_state_dict=True)),
        ('gauss_t1_nomean', dict(S=3, C=4, M=20, D=2, B=100, n_prev=1, seed=304, kind='wtoy', beta=1.0, n_total=100,
                                 ep_var_mean=False)),
        # 20 outputs (beyond the softmax kernels' 16-class tile); M > 104 (first task on the block program)
        ('gauss_c20_t0', dict(S=2, C=20, M=16, D=8, B=64, n_prev=0, seed=305, kind='gauss', beta=2.0, n_total=640)),
        ('gauss_m112_t0', dict(S=2, C=3, M=112, D=8, B=64, n_prev=0, seed=306, kind='gauss', beta=2.0, n_total=640)),
        # BASELINE config 2's shape (S3 C10 M100 D784 B512), first task: outputs only, inputs regenerated from the seed
        ('gauss_full_t0', dict(S=3, C=10, M=100, D=784, B=512, n_prev=0, seed=307, kind='gauss', beta=10.0, n_total=12000,
                               store_inputs=False)),
    ]
    for name, kw in cases:
        if not only or name in only:
            gauss_case(name, **kw)
    if not only or 'retrain_gauss_wtoy_t1' in only:
        retrain_gauss_case('retrain_gauss_wtoy_t1', 2, 3, 12, 2, 64, 1, 308, 'wtoy', beta=1.0, n_total=64)
