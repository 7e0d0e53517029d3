"""The gradient of the pathwise function samples in their inputs on the device: ops.rff_paths_x (csrc/rff.hip,
vargp_rff_paths_bwd), PosteriorPaths.differentiable and PosteriorPaths.ascend against autograd of the fp64 references of
tests/test_hip_paths.py (pinned on the host by tests/test_paths_grad.py).

Rule, per case:  err(HIP, fp64) <= RTOL_SCALAR + 2 err(torch fp32 on one host thread, fp64), with err = max |g - g_64| / max |g_64|
over the gradient of the case; the host error itself is capped at HOST_CAP = 1e-3, so that the rule never turns vacuous.
Frequencies: N(0, I) and the Matern-5/2 law.  (Not the Matern-1/2 inputs of the forward test: their fp32 HOST gradient is off
by up to 5e-2 -- the Cauchy tail puts the gradient on a few features with phases of thousands of radians, which tests the fp32
rounding of the phases and not the kernel.)  Host errors of the op cases, measured on the CPU: at most 5.9e-6 ('normal') and
6.5e-5 ('matern52') in the sweep, 4.3e-6 in the tile cases; of the model cases: at most 8.2e-6."""
import functools
import itertools

import pytest
import torch

from helpers import RTOL_SCALAR, to_dev
from test_hip_paths import (HOST_CAP, KERNELS, N_FEAT, N_PATHS, TILE_CASES, _case, _gp, _ref)
from test_hip_predict_f import _one_thread
from test_paths_grad import grad_autograd, grad_inputs
from test_predict_f import SHAPES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _rel(g, g64):
    return ((g.cpu().double() - g64).abs().max() / g64.abs().max()).item()


# -- a, b. the op -----------------------------------------------------------------------------------------------------------------
def _op_host(n, D, R, N, shared, kind, seed):
    """-> inputs (with gout), the fp64 gradient, the fp32 host error."""
    inp = grad_inputs(n, D, R, N, shared, kind, seed)
    g64 = grad_autograd(*inp, shared, torch.float64)
    g32 = _one_thread(lambda: grad_autograd(*inp, shared, torch.float32))
    return inp, g64, _rel(g32, g64)


def _op_case(n, D, R, N, shared, kind, seed):
    """-> (err_hip, err_32, messages) of one case."""
    from vargp_amd import ops
    inp, g64, e_32 = _op_host(n, D, R, N, shared, kind, seed)
    theta, X, omega, coef, gout = (t.to(DEV) for t in inp)
    grads, outs = [], []
    for _ in range(2):
        x = X.detach().clone().requires_grad_(True)
        out = ops.rff_paths_x(theta, x, omega, coef, shared)
        outs.append(out.detach())
        grads.append(torch.autograd.grad(out, x, gout)[0])
    got = grads[0]
    assert got.shape == g64.shape and got.dtype == torch.float32
    e_hip = _rel(got, g64)
    tag = f'n{n} D{D} R{R} N{N} shared={int(shared)} {kind}'
    msgs = []
    if not e_32 <= HOST_CAP:
        msgs.append(f'{tag}: fp32 host error {e_32:.2e} above the cap {HOST_CAP:.0e}')
    if not e_hip <= RTOL_SCALAR + 2.0 * e_32:
        msgs.append(f'{tag}: err {e_hip:.2e} > {RTOL_SCALAR:.0e} + 2 x {e_32:.2e}')
    if not torch.equal(grads[0], grads[1]):
        msgs.append(f'{tag}: two backward calls differ')
    if not (torch.equal(outs[0], ops.rff_paths(theta, X, omega, coef, shared)) and torch.equal(outs[0], outs[1])):
        msgs.append(f'{tag}: the forward is not rff_paths bit for bit')
    return e_hip, e_32, msgs


NS, DS, RS, NPS = (1, 31, 33, 65, 130), (2, 33, 70, 300), (1, 32, 33, 100), (1, 3, 17)
SEED0 = {'normal': 5000, 'matern52': 7000}


@pytest.mark.parametrize('kind', ['normal', 'matern52'])
@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per-output'])
def test_op_grad_vs_fp64(shared, kind):
    """Full cross product of the sizes (240 cases, S x C = 2 x 3; D = 2 | 33 one 64-wide tile, 70 one 128-wide, 300 two 256-wide,
    the second ragged) against fp64 by the rule; two calls bitwise equal; the forward is rff_paths."""
    bad, worst, host = [], (0.0, None), 0.0
    for i, (n, D, R, N) in enumerate(itertools.product(NS, DS, RS, NPS)):
        e_hip, e_32, msgs = _op_case(n, D, R, N, shared, kind, seed=SEED0[kind] + i)
        bad += msgs
        host = max(host, e_32)
        r = e_hip / (RTOL_SCALAR + 2.0 * e_32)
        if r > worst[0]:
            worst = (r, f'n{n} D{D} R{R} N{N}: err {e_hip:.2e}, fp32 host {e_32:.2e}')
    print(f'shared={int(shared)} {kind}: worst case {worst[1]} ({worst[0]:.3f} of the bound); largest fp32 host error {host:.2e}')
    assert not bad, bad


# the contraction widths C N (or N) of gout coef^T -- 51, 17, 90, 270, 70, 260 columns, slabs of 16 -- and the D-tile edges:
# D = 300 with 260 columns, D = 784 = three 256-wide tiles and one of 16
GRAD_TILE_CASES = TILE_CASES + [(70, 300, 33, 260, False), (70, 784, 64, 4, True)]


@pytest.mark.parametrize('n,D,R,N,shared', GRAD_TILE_CASES)
def test_op_grad_tiles(n, D, R, N, shared):
    e_hip, e_32, msgs = _op_case(n, D, R, N, shared, 'normal', seed=77 + n + N)
    print(f'n{n} D{D} R{R} N{N} shared={int(shared)}: err {e_hip:.2e}, fp32 host {e_32:.2e}')
    assert not msgs, msgs


def test_op_grad_bad_arguments():
    """Every check below fails before anything is launched, so the small tensors behind the pointers are never indexed."""
    from vargp_amd._lib import VargpHipError, check, lib, ptr, stream_ptr
    S, C, n, D, R, N = 2, 3, 5, 4, 6, 2
    t = [torch.zeros(k, device=DEV) for k in (S * (D + 1), C * n * D, R * D, S * C * 2 * R * N, S * C * n * N, C * n * D)]
    need = lib().vargp_rff_paths_bwd_workspace_bytes(S, C, n, D, R, 0)
    ws = torch.zeros(need // 4 + 1, device=DEV)

    def call(S, C, n, D, R, N, shared, ws_bytes):
        check(lib().vargp_rff_paths_bwd(*(ptr(a) for a in t), S, C, n, D, R, N, shared, ptr(ws), ws_bytes, stream_ptr()),
              'vargp_rff_paths_bwd')

    call(S, C, n, D, R, N, 0, need)                                  # (the well-formed call passes)
    torch.cuda.synchronize()
    with pytest.raises(VargpHipError):
        call(S, C, n, D, R, N, 0, need - 4)                          # workspace too small
    with pytest.raises(VargpHipError):
        call(S, C, n, D, R, N, 2, need)                              # x_shared neither 0 nor 1
    with pytest.raises(VargpHipError):
        call(1, 65536, 1, 1, 1, 1, 1, need)                          # S C above the grid limit
    with pytest.raises(VargpHipError):
        call(1, 2, 1 << 15, 1 << 15, 1, 1, 0, need)                  # gX (C, n, D) of 2^31 elements
    with pytest.raises(VargpHipError):
        call(1, 1, 1 << 16, 1 << 15, 1, 1, 1, need)                  # n D = 2^31


# -- d. the model -----------------------------------------------------------------------------------------------------------------
# The deep-kernel case is evaluated at 0.9 x: at x itself point 27 sits on a kink of the feature map (a second-layer pre-activation
# of 2.4e-8 against a typical 0.17), the fp32 host evaluation takes the other side of the ReLU there and its gradient of that row
# is off by 1e-3 .. 7e-2 of max |g_64|, depending on w -- above the cap, and a statement about the kink, not about any kernel.  At
# 0.9 x (picked on the CPU) the host gradient error is 1.1e-6.
DKL_CASE = ('dkl', (2, 3, 3, 20, 40, 36), 1)
DKL_XSCALE = 0.9


def _weights(shape):
    S, C, B = shape[0], shape[2], shape[5]
    return torch.randn(N_PATHS, S, C, B, generator=torch.Generator().manual_seed(41 + B))


def _ref_grad(prob, w, dtype):
    x = prob[2].detach().to(dtype).clone().requires_grad_(True)
    f, _ = _ref(prob[:2] + (x,) + prob[3:], dtype)
    return torch.autograd.grad((f * w.to(dtype)).sum(), x)[0]


@functools.lru_cache(maxsize=None)
def _grad_case(kern, shape, n_prev, xscale=1.0):
    """The case of test_hip_paths._case (at xscale x, with its fp64 values and their fp32 host error) with the weights w, the fp64
    gradient of (f w).sum() in x through ref_paths and the fp32 host error of that gradient -- computed once, shared, left
    unchanged."""
    prob, f64, gamma, e_32 = _case(kern, shape, n_prev)
    if xscale != 1.0:
        prob = prob[:2] + (prob[2] * xscale,) + prob[3:]
        f64 = _ref(prob, torch.float64)[0]
        e_32 = ((_one_thread(lambda: _ref(prob, torch.float32))[0].double() - f64).abs() / gamma).max().item()
    w = _weights(shape)
    g64 = _ref_grad(prob, w, torch.float64)
    g32 = _one_thread(lambda: _ref_grad(prob, w, torch.float32))
    return prob, f64, gamma, e_32, w, g64, _rel(g32, g64)


def _paths(prob, kern, shape):
    from vargp_amd import noise
    gp = _gp(prob, kern, shape)
    with noise.inject(**to_dev(prob[4], DEV)):
        return gp.sample_paths(n_paths=N_PATHS, n_features=N_FEAT)


def _model_grad(kern, shape, n_prev, xscale=1.0):
    prob, f64, gamma, e_32, w, g64, eg_32 = _grad_case(kern, shape, n_prev, xscale)
    paths = _paths(prob, kern, shape)
    x = prob[2].detach().to(DEV).requires_grad_(True)
    f = paths.differentiable(x)
    S, C, B = shape[0], shape[2], shape[5]
    assert f.shape == (N_PATHS, S, C, B) and f.dtype == torch.float32 and f.requires_grad
    (f * w.to(DEV)).sum().backward()
    assert x.grad.shape == x.shape
    eg_hip = _rel(x.grad, g64)
    bound_f = RTOL_SCALAR + 2.0 * e_32
    e_val = ((f.detach().cpu() - paths(x.detach()).cpu()).abs() / gamma.float()).max().item()
    e_f = ((f.detach().cpu().double() - f64).abs() / gamma).max().item()
    print(f'{kern} {shape} n_prev={n_prev}: gradient err {eg_hip:.2e} (fp32 host {eg_32:.2e}); differentiable(x) vs paths(x) '
          f'{e_val:.2e}, vs fp64 {e_f:.2e} (fp32 host {e_32:.2e})')
    assert e_32 <= HOST_CAP and eg_32 <= HOST_CAP
    assert eg_hip <= RTOL_SCALAR + 2.0 * eg_32, (eg_hip, eg_32)
    assert e_val <= bound_f and e_f <= bound_f
    frozen = dict(theta=paths.theta, V=paths.V, z=paths.z, omega=paths.omega, coef=paths.coef, **dict(paths.kernel.named_parameters()))
    assert all(t.grad is None and not t.requires_grad for t in frozen.values()), [k for k, t in frozen.items() if t.grad is not None]


@pytest.mark.parametrize('n_prev', [0, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'M%d-D%d-B%d' % s[3:])
@pytest.mark.parametrize('kern', KERNELS[:3])
def test_differentiable_vs_fp64(kern, shape, n_prev):
    _model_grad(kern, shape, n_prev)


def test_differentiable_deep_kernel():
    _model_grad(*DKL_CASE, xscale=DKL_XSCALE)


# -- e. ascend --------------------------------------------------------------------------------------------------------------------
def test_ascend():
    """Eight ascents of one sampled function (rbf, D = 2, first task), 20 steps of 0.05 l^2 / max |grad f| (l the smallest
    lengthscale of the hyper-sample, the gradient taken at the starts): a step far inside the lengthscale, along the slope, so
    the function does not decrease at any start; and the returned values are the function at the returned points."""
    kern, shape, n_prev = 'rbf', SHAPES[0], 0
    assert shape[4] == 2
    prob, _, gamma, e_32 = _case(kern, shape, n_prev)
    paths = _paths(prob, kern, shape)
    index = (1, 1, 2)
    k, s, c = index
    x0 = prob[2][:8].to(DEV)
    xg = x0.clone().requires_grad_(True)
    f0 = paths.differentiable(xg)[index]
    grad0 = torch.autograd.grad(f0.sum(), xg)[0]
    ell = paths.theta[s, :-1].exp().min().item()
    step = 0.05 * ell ** 2 / grad0.abs().max().item()
    x, fx = paths.ascend(x0, index, n_steps=20, step_size=step)
    assert x.shape == x0.shape and fx.shape == (8,) and not x.requires_grad and not fx.requires_grad
    assert torch.equal(x0, prob[2][:8].to(DEV))                      # the starts are left alone
    bound = RTOL_SCALAR + 2.0 * e_32
    e_val = ((fx - paths(x)[index]).abs().max() / gamma[0, s, 0, 0].float()).item()
    gain = (fx - f0.detach()).cpu()
    moved = (x - x0).norm(dim=-1).cpu()
    print(f'step {step:.3e} (l = {ell:.3f}); f(x) - f(x0) in [{gain.min().item():.3e}, {gain.max().item():.3e}]; |x - x0| up to '
          f'{moved.max().item():.3e}; f(x) vs paths(x) {e_val:.2e} (bound {bound:.2e})')
    assert e_32 <= HOST_CAP and e_val <= bound
    assert moved.max().item() > 0
    assert (gain >= 0).all(), gain
