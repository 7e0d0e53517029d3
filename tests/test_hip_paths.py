"""Pathwise function samples on the device: ops.rff_paths (csrc/rff.hip) and VARGP.sample_paths (vargp_amd/paths.py) against the
fp64 reference of tests/test_paths.py.

Rule (tests/test_hip_predict_f.py), per case:  err(HIP, fp64) <= RTOL_SCALAR + 2 err(torch fp32 on the host, fp64), with
err = max |a - a_64| / gamma_s, the scale of a function value of hyper-sample s.  The fp32 host evaluation runs on one thread
(sweep_rule.py), and its own error is capped at 1e-3 in every case, so that the rule never turns vacuous: the phases are
rounded to fp32 whoever evaluates them, and a case whose phases are so large that this rounding alone spoils the result would
prove nothing about the kernel."""
import functools
import itertools
import math

import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import RTOL_SCALAR, to_dev
from test_hip_predict_f import _one_thread, matern_gram
from test_paths import ref_paths, ref_phi
from test_predict_f import SHAPES, ref_predict_f

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S_OP, C_OP = 2, 3
HOST_CAP = 1e-3


def _matern_omega(g, mix):
    nu2 = mix.shape[-1]
    return g * (nu2 / (mix ** 2).sum(-1, keepdim=True)).sqrt()


# -- 1. the op --------------------------------------------------------------------------------------------------------------------
def _op_inputs(n, D, R, N, shared, kind, seed, S=S_OP, C=C_OP):
    """theta, X, omega, coef (fp32, host).  kind 'normal': omega ~ N(0, I) and points of squared norm ~25 at lengthscales ~0.5,
    phases of tens of radians (up to ~100).  kind 'matern12': the heavy-tailed Matern-1/2 (Cauchy) frequencies; a phase is then
    |x / lengthscale| times a standard Cauchy variable, whose largest of the up to 130 x 100 draws of a case is of the order of
    1e4, so the points have squared norm ~0.01 (|x / lengthscale| ~ 0.2): phases up to a few thousand radians, where their
    fp32 rounding (|p| 2^-24 per feature, times |coef| / sqrt(R)) still leaves the fp32 host result under its cap of 1e-3."""
    g = torch.Generator().manual_seed(seed)
    theta = math.log(0.5) + 0.05 * torch.randn(S, D + 1, generator=g)
    X = torch.randn(*(() if shared else (C,)), n, D, generator=g) * math.sqrt((0.01 if kind == 'matern12' else 25.0) / D)
    omega = torch.randn(R, D, generator=g)
    if kind == 'matern12':
        omega = _matern_omega(omega, torch.randn(R, 1, generator=g))
    coef = torch.randn(S, C, 2 * R, N, generator=g)
    return theta, X, omega, coef


def _op_formula(theta, X, omega, coef, shared, dtype):
    theta, X, omega, coef = theta.to(dtype), X.to(dtype), omega.to(dtype), coef.to(dtype)
    Phi = ref_phi(theta, X, omega)                        # (S, n, 2R) | (S, C, n, 2R)
    return (Phi.unsqueeze(1) if shared else Phi) @ coef


def _op_host(n, D, R, N, shared, kind, seed, **kw):
    """-> inputs, fp64 result, fp32 host error (the part of a case that needs no device)."""
    inp = _op_inputs(n, D, R, N, shared, kind, seed, **kw)
    s64 = _op_formula(*inp, shared, torch.float64)
    s32 = _one_thread(lambda: _op_formula(*inp, shared, torch.float32))
    gamma = inp[0][:, -1].double().exp().view(-1, 1, 1, 1)
    return inp, s64, gamma, ((s32.double() - s64).abs() / gamma).max().item()


def _op_case(n, D, R, N, shared, kind, seed, **kw):
    """-> (err_hip, err_32, messages) of one case."""
    from vargp_amd import ops
    inp, s64, gamma, e_32 = _op_host(n, D, R, N, shared, kind, seed, **kw)
    dev = [t.to(DEV) for t in inp]
    got = ops.rff_paths(*dev, shared)
    again = ops.rff_paths(*dev, shared)
    assert got.shape == s64.shape and got.dtype == torch.float32
    e_hip = ((got.cpu().double() - s64).abs() / gamma).max().item()
    tag = f'n{n} D{D} R{R} N{N} shared={int(shared)} {kind}'
    msgs = []
    if not e_32 <= HOST_CAP:
        msgs.append(f'{tag}: fp32 host error {e_32:.2e} above the cap {HOST_CAP:.0e}')
    if not e_hip <= RTOL_SCALAR + 2.0 * e_32:
        msgs.append(f'{tag}: err {e_hip:.2e} > {RTOL_SCALAR:.0e} + 2 x {e_32:.2e}')
    if not torch.equal(got, again):
        msgs.append(f'{tag}: two calls differ')
    return e_hip, e_32, msgs


NS, DS, RS, NPS = (1, 31, 33, 65, 130), (2, 33, 40), (1, 32, 33, 100), (1, 3, 17)


@pytest.mark.parametrize('kind', ['normal', 'matern12'])
@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per-output'])
def test_op_vs_fp64(shared, kind):
    """Full cross product of the sizes (180 cases, S x C = 2 x 3) against fp64 by the sweep rule; two calls bitwise equal."""
    bad, worst, host = [], (0.0, None), 0.0
    for i, (n, D, R, N) in enumerate(itertools.product(NS, DS, RS, NPS)):
        e_hip, e_32, msgs = _op_case(n, D, R, N, shared, kind, seed=1000 * (kind == 'matern12') + i)
        bad += msgs
        host = max(host, e_32)
        r = e_hip / (RTOL_SCALAR + 2.0 * e_32)
        if r > worst[0]:
            worst = (r, f'n{n} D{D} R{R} N{N}: err {e_hip:.2e}, fp32 host {e_32:.2e}')
    print(f'shared={int(shared)} {kind}: worst case {worst[1]} ({worst[0]:.3f} of the bound); largest fp32 host error {host:.2e}')
    assert not bad, bad


# the widths at which the second product changes its tile (csrc/rff.hip: 64 WN columns, WN = 1 | 2 | 4, then 256-wide tiles side by
# side): n = 300 is five 64-point tiles, the last one ragged; N C = 51 is the issue's case (one 64-wide tile here); 90 takes the
# 128-wide, 270 two 256-wide tiles, the second one ragged -- per-output point sets reach the same widths through N alone
TILE_CASES = [(300, 40, 100, 17, True), (300, 40, 100, 17, False), (130, 33, 33, 30, True), (130, 33, 33, 90, True),
              (70, 33, 33, 70, False), (70, 2, 33, 260, False)]


@pytest.mark.parametrize('n,D,R,N,shared', TILE_CASES)
def test_op_tiles(n, D, R, N, shared):
    e_hip, e_32, msgs = _op_case(n, D, R, N, shared, 'normal', seed=77 + n + N)
    print(f'n{n} D{D} R{R} N{N} shared={int(shared)}: err {e_hip:.2e}, fp32 host {e_32:.2e}')
    assert not msgs, msgs


def test_op_bad_arguments():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    C = 65536                                            # S C above the grid limit
    with pytest.raises(VargpHipError):
        ops.rff_paths(torch.zeros(1, 2, device=DEV), torch.zeros(1, 1, device=DEV), torch.zeros(1, 1, device=DEV),
                      torch.zeros(1, C, 2, 1, device=DEV), True)


# -- 2. the model -----------------------------------------------------------------------------------------------------------------
N_PATHS, N_FEAT = 4, 64
KERNELS = ['rbf', 'matern52', 'matern52-native', 'dkl']


def _fill(gp, params):
    with torch.no_grad():
        gp.kernel.log_mean.copy_(params['log_mean'])
        gp.kernel.log_logvar.copy_(params['log_logvar'])
        gp.u_mean.copy_(params['u_mean'])
        gp.u_tril_vec.copy_(params['u_tril_vec'])
    return gp.to(DEV)


def _problem(kern, shape, n_prev):
    """-> params, prev, x, y, noise (all of it, by name), nu2, phi of a case; host tensors."""
    S, F_, C, M, D, B = shape
    phi, nu2, Df = None, 5 if kern.startswith('matern52') else 0, D
    if kern == 'dkl':
        params, prev, x, y, nz, phi = orc.make_dkl_problem(S, F_, C, M, D, B, n_prev, seed=21)
        Df = phi['4.weight'].shape[0]
    else:
        params, prev, x, y, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=n_prev, seed=5 + n_prev, kind='wtoy' if D == 2 else 'gauss')
    g = torch.Generator().manual_seed(31 + n_prev + D)
    Mt = (n_prev + 1) * M
    nz = dict(eps_theta=nz['eps_theta'], rff_omega=torch.randn(N_FEAT, Df, generator=g),
              rff_w=torch.randn(S, C, 2 * N_FEAT, N_PATHS, generator=g), eps_up=torch.randn(S, C, Mt, N_PATHS, generator=g))
    if nu2:
        nz['rff_mix'] = torch.randn(N_FEAT, nu2, generator=g)
    return params, prev, x, y, nz, nu2, phi


def _build(kern, params, prev, shape):
    from vargp_amd.kernels import DeepRBFKernel, MaternKernel, RBFKernel
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.vargp import VARGP
    S, F_, C, M, D, B = shape
    hp = dict(prior_log_mean=params['prior_log_mean'], prior_log_logvar=params['prior_log_logvar'])
    if kern == 'dkl':
        k = DeepRBFKernel(D, **hp)
    elif kern.startswith('matern52'):
        k = MaternKernel(D, nu=2.5, native=kern.endswith('native'), **hp)
    else:
        k = RBFKernel(D, **hp)
    return VARGP(params['z'], k, MulticlassSoftmax(n_f=F_), n_var_samples=S, prev_params=[{a: v.clone() for a, v in p.items()} for p in prev])


def _with_kernel(nu2, phi, dtype, fn):
    """fn() with the case's kernel in place of the oracle's RBF."""
    with pytest.MonkeyPatch.context() as m:
        if nu2:
            m.setattr(orc, 'rbf_gram', lambda theta, x, y=None, full_gram=False: matern_gram(theta, x, y, nu2=nu2))
        if phi is not None:
            with orc.deep_kernel({k: v.to(dtype) for k, v in phi.items()}):
                return fn()
        return fn()


def _ref(prob, dtype, coef=None, eps_u=None):
    params, prev, x, _, nz, nu2, phi = prob
    omega = nz['rff_omega'].to(dtype)
    if nu2:
        omega = _matern_omega(omega, nz['rff_mix'].to(dtype))
    coef = nz['rff_w'] if coef is None else coef
    eps_u = nz['eps_up'] if eps_u is None else eps_u
    return _with_kernel(nu2, phi, dtype, lambda: ref_paths(params, prev, x, nz, omega, coef, eps_u, dtype))


@functools.lru_cache(maxsize=None)
def _case(kern, shape, n_prev):
    """The problem, the fp64 reference f64 (N, S, C, B), gamma (1, S, 1, 1) and the fp32 host error of a case -- computed once
    and shared by the tests below, which leave it unchanged."""
    prob = _problem(kern, shape, n_prev)
    f64, theta = _ref(prob, torch.float64)
    f32, _ = _one_thread(lambda: _ref(prob, torch.float32))
    gamma = theta[:, -1].exp().view(1, -1, 1, 1)
    e_32 = ((f32.double() - f64).abs() / gamma).max().item()
    return prob, f64, gamma, e_32


def _gp(prob, kern, shape):
    params, prev, _, _, _, _, phi = prob
    gp = _build(kern, params, prev, shape)
    if phi is not None:
        gp.kernel.phi.load_state_dict(phi)
    return _fill(gp, params)


def _err(a, f64, gamma):
    return ((a.cpu().double() - f64).abs() / gamma).max().item()


@pytest.mark.parametrize('n_prev', [0, 2])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'M%d-D%d-B%d' % s[3:])
@pytest.mark.parametrize('kern', KERNELS[:3])
def test_sample_paths_vs_fp64(kern, shape, n_prev):
    from vargp_amd import noise
    prob, f64, gamma, e_32 = _case(kern, shape, n_prev)
    gp, x = _gp(prob, kern, shape), prob[2].to(DEV)
    with noise.inject(**to_dev(prob[4], DEV)):
        paths = gp.sample_paths(n_paths=N_PATHS, n_features=N_FEAT)
    f = paths(x)
    S, C, B = shape[0], shape[2], shape[5]
    assert f.shape == (N_PATHS, S, C, B) and f.dtype == torch.float32 and not f.requires_grad
    assert paths.n_paths == N_PATHS and paths.n_features == N_FEAT and paths.theta.shape == (S, shape[4] + 1)
    e_hip = _err(f, f64, gamma)
    print(f'{kern} {shape} n_prev={n_prev}: err {e_hip:.2e} (fp32 host {e_32:.2e}); max |f| / gamma {(f64.abs() / gamma).max().item():.1f}')
    assert e_32 <= HOST_CAP
    assert e_hip <= RTOL_SCALAR + 2.0 * e_32, (e_hip, e_32)


def test_sample_paths_deep_kernel():
    from vargp_amd import noise
    kern, shape, n_prev = 'dkl', (2, 3, 3, 20, 40, 36), 1
    prob, f64, gamma, e_32 = _case(kern, shape, n_prev)
    gp, x = _gp(prob, kern, shape), prob[2].to(DEV)
    with noise.inject(**to_dev(prob[4], DEV)):
        f = gp.sample_paths(n_paths=N_PATHS, n_features=N_FEAT)(x)
    e_hip = _err(f, f64, gamma)
    print(f'dkl: err {e_hip:.2e} (fp32 host {e_32:.2e})')
    assert e_32 <= HOST_CAP
    assert e_hip <= RTOL_SCALAR + 2.0 * e_32, (e_hip, e_32)


def test_paths_are_functions():
    """One draw is one set of functions: blocks, subsets and repeated calls evaluate the same ones, and training the model
    afterwards does not change them."""
    from vargp_amd import noise
    kern, shape, n_prev = 'rbf', SHAPES[1], 2
    prob, f64, gamma, e_32 = _case(kern, shape, n_prev)
    gp, x, y = _gp(prob, kern, shape), prob[2].to(DEV), prob[3].to(DEV)
    nz = to_dev(prob[4], DEV)
    with noise.inject(**nz):
        paths = gp.sample_paths(n_paths=N_PATHS, n_features=N_FEAT)
    f = paths(x)
    bound = RTOL_SCALAR + 2.0 * e_32
    assert e_32 <= HOST_CAP
    g = gamma.float()
    e_tile = ((paths(x, tile=16).cpu() - f.cpu()).abs() / g).max().item()
    e_sub = ((paths(x[:10]).cpu() - f[..., :10].cpu()).abs() / g).max().item()
    print(f'tile=16 vs one block {e_tile:.2e}; x[:10] vs the first 10 of x {e_sub:.2e}; bound {bound:.2e}')
    assert e_tile <= bound and e_sub <= bound
    assert _err(paths(x, tile=16), f64, gamma) <= bound
    assert torch.equal(paths(x), f)

    # an optimiser step moves every parameter; the sampled functions stay where they are
    before = [p.detach().clone() for p in gp.parameters()]
    opt = torch.optim.Adam(gp.parameters(), lr=1e-3)      # every entry moves by ~1e-3 whatever the scale of its gradient
    kl_h, kl_u, nll = gp.loss(x, y)
    (kl_h + kl_u + nll).backward()
    opt.step()
    torch.cuda.synchronize()
    assert all(not torch.equal(a, b) for a, b in zip(before, gp.parameters()))
    assert torch.equal(paths(x), f)
    with noise.inject(**nz):                              # (and a new draw from the moved model is another function)
        assert not torch.equal(gp.sample_paths(n_paths=N_PATHS, n_features=N_FEAT)(x), f)


@pytest.mark.parametrize('n_prev', [0, 2])
def test_zero_noise_is_the_predictive_mean(n_prev):
    from vargp_amd import noise
    kern, shape = 'rbf', SHAPES[1]
    prob = _case(kern, shape, n_prev)[0]
    params, prev, x, _, nz, _, _ = prob
    gp, xd = _gp(prob, kern, shape), x.to(DEV)
    zero = dict(nz, rff_w=torch.zeros_like(nz['rff_w']), eps_up=torch.zeros_like(nz['eps_up']))
    mu64, _, theta = ref_predict_f(params, prev, x, nz)
    mu32, _, _ = _one_thread(lambda: ref_predict_f(params, prev, x, nz, torch.float32))
    gamma = theta[:, -1].exp().view(-1, 1, 1)
    e_32 = ((mu32.double() - mu64).abs() / gamma).max().item()
    with noise.inject(**to_dev(zero, DEV)):
        f = gp.sample_paths(n_paths=N_PATHS, n_features=N_FEAT)(xd)
        mu = gp.predict_f(xd)[0]
    e_ref = max(_err(f[k], mu64, gamma) for k in range(N_PATHS))
    e_dev = ((f.cpu() - mu.cpu().unsqueeze(0)).abs() / gamma.float()).max().item()
    print(f'n_prev={n_prev}: paths at zero noise vs fp64 mean {e_ref:.2e}, vs predict_f on the device {e_dev:.2e} (fp32 host {e_32:.2e})')
    assert e_32 <= HOST_CAP
    assert e_ref <= RTOL_SCALAR + 2.0 * e_32 and e_dev <= RTOL_SCALAR + 2.0 * e_32
