"""The gradient of the random-Fourier-feature paths in their points -- what ops.rff_paths_x (csrc/rff.hip, vargp_rff_paths_bwd)
computes -- written out in fp64 and pinned to torch.autograd.grad of the forward formula (test_hip_paths._op_formula), which is
the reference of tests/test_hip_paths_grad.py:

    om[s, r, d] = omega[r, d] / ell[s, d],   gs[s] = gamma_s / sqrt(R),   p[s, i, r] = sum_d X[i, d] om[s, r, d]
    h[s, i, r]  = sum_(c, k) gout[s, c, i, k] (-sin p[s, i, r] coef[s, c, r, k] + cos p[s, i, r] coef[s, c, R + r, k])
    gX[i, d]    = sum_s gs[s] sum_r h[s, i, r] om[s, r, d]

(per-output point sets: the sum in h runs over k only, on output c's points, and gX keeps its c index).  No device needed."""
import math

import pytest
import torch

from test_hip_paths import _matern_omega, _op_formula, _op_inputs


def grad_formula(theta, X, omega, coef, gout, shared, dtype=torch.float64):
    """gX (n, D) | (C, n, D) by the formula above, in `dtype`."""
    theta, X, omega, coef, gout = (t.to(dtype) for t in (theta, X, omega, coef, gout))
    R = omega.shape[0]
    om = omega.unsqueeze(0) / theta[:, :-1].exp().unsqueeze(1)                   # (S, R, D)
    gs = theta[:, -1].exp() / math.sqrt(R)                                       # (S,)
    if shared:
        p = torch.einsum('id,srd->sir', X, om)
        h = torch.einsum('scik,scrk->sir', gout, coef[:, :, :R]) * -p.sin() + torch.einsum('scik,scrk->sir', gout, coef[:, :, R:]) * p.cos()
        return torch.einsum('s,sir,srd->id', gs, h, om)
    p = torch.einsum('cid,srd->scir', X, om)
    h = torch.einsum('scik,scrk->scir', gout, coef[:, :, :R]) * -p.sin() + torch.einsum('scik,scrk->scir', gout, coef[:, :, R:]) * p.cos()
    return torch.einsum('s,scir,srd->cid', gs, h, om)


def grad_autograd(theta, X, omega, coef, gout, shared, dtype):
    """gX by torch.autograd.grad of _op_formula in `dtype`."""
    x = X.detach().to(dtype).clone().requires_grad_(True)
    out = _op_formula(theta, x, omega, coef, shared, dtype)
    return torch.autograd.grad(out, x, gout.to(dtype))[0]


def grad_inputs(n, D, R, N, shared, kind, seed, S=2, C=3):
    """theta, X, omega, coef of _op_inputs(..., 'normal', seed) -- kind 'matern52': the same points with the Matern-5/2
    frequencies -- and gout (S, C, n, N) ~ N(0, 1)."""
    theta, X, omega, coef = _op_inputs(n, D, R, N, shared, 'normal', seed, S=S, C=C)
    g = torch.Generator().manual_seed(seed + 500000)
    mix = torch.randn(R, 5, generator=g)
    if kind == 'matern52':
        omega = _matern_omega(omega, mix)
    else:
        assert kind == 'normal', kind
    return theta, X, omega, coef, torch.randn(S, C, n, N, generator=g)


def test_new_entries_are_bound():
    from vargp_amd import _lib, ops
    from vargp_amd.paths import PosteriorPaths
    assert {'vargp_rff_paths_bwd', 'vargp_rff_paths_bwd_workspace_bytes'} <= set(_lib.EXPORTS)
    assert callable(ops.rff_paths_x) and callable(PosteriorPaths.differentiable) and callable(PosteriorPaths.ascend)
    S, C, n, D, R = 2, 3, 130, 40, 100
    lib = _lib.lib()
    # the pre-scaled frequencies and amplitudes of the forward, and room for one partial sum per hyper-sample at least
    fwd = lib.vargp_rff_paths_workspace_bytes(S, D, R)
    assert lib.vargp_rff_paths_bwd_workspace_bytes(S, C, n, D, R, 1) >= fwd + 4 * S * n * D
    assert lib.vargp_rff_paths_bwd_workspace_bytes(S, C, n, D, R, 0) >= fwd + 4 * S * C * n * D
    assert lib.vargp_rff_paths_bwd_workspace_bytes(1, C, n, D, 1, 1) >= lib.vargp_rff_paths_workspace_bytes(1, D, 1)
    assert lib.vargp_rff_paths_bwd_workspace_bytes(0, C, n, D, R, 1) == 0


def test_rff_paths_x_refuses_cpu_tensors():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    S, C, n, D, R, N = 2, 3, 5, 4, 6, 2
    for shared in (True, False):
        X = torch.zeros(*(() if shared else (C,)), n, D, requires_grad=True)
        with pytest.raises(VargpHipError):
            ops.rff_paths_x(torch.zeros(S, D + 1), X, torch.zeros(R, D), torch.zeros(S, C, 2 * R, N), shared)


@pytest.mark.parametrize('kind', ['normal', 'matern52'])
@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per-output'])
@pytest.mark.parametrize('n,D,R,N', [(1, 2, 1, 1), (33, 33, 32, 3), (65, 70, 33, 17), (31, 300, 100, 3)])
def test_formula_is_the_gradient_of_the_forward(n, D, R, N, shared, kind):
    inp = grad_inputs(n, D, R, N, shared, kind, seed=11 + n + D)
    want = grad_autograd(*inp, shared, torch.float64)
    got = grad_formula(*inp, shared)
    assert got.shape == inp[1].shape and got.dtype == torch.float64
    err = ((got - want).abs().max() / want.abs().max()).item()
    print(f'n{n} D{D} R{R} N{N} shared={int(shared)} {kind}: formula vs autograd {err:.2e}')
    assert err <= 1e-10
