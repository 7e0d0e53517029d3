"""PoissonLikelihood and StudentTLikelihood (csrc/indep_lik.hip; not in the reference, so no reference goldens).  Yardstick at op
level: the fp64 restatements `poisson_ell` / `studentt_ell` below (the closed form, and the 20-node Gauss-Hermite sum that DEFINES
the Student-t expectation) with torch.autograd.  At model level: the composed per-op route of the same model.

Op-level bounds.  Typical inputs: the project's op-level bound (tests/test_hip_bernoulli.py): value within
1e-5 x sum|terms| / S, rel_l2 < 1e-5 per gradient, g_log_scale included.  Edge inputs: the same formula is evaluated in fp32
torch on the CPU on the same case and the kernel's error against fp64 may be at most 4 x that error (the factor 4 for a
different summation order) -- no floor under it.  The bound comes from that independent implementation, never from the kernel.
Edge kinds are chosen so that the fp32 restatement keeps a digit in EVERY case (asserted: nothing is left out of the table).
Student-t at var = 0: torch's autograd of sqrt(2 var) is 0 x inf there, so the variance gradient has no autograd yardstick; the
kernel's is DEFINED as exactly 0 (the pair differences vanish) and is checked to be that; value, gmu and g_log_scale are checked
against fp64 as everywhere else.
Each edge kind runs with one target form ((C, B) and the shared row alternate over the kinds); typical inputs run with both.

The bound has no floor, and an fp32 result can land within 1e-10 of the exact value by chance, so it can only be met by
rounding once: the kernels take and return fp32 but evaluate an element and every sum in fp64 (csrc/indep_lik.hip), which makes
each output the nearest fp32 to the formula's value -- never further from it than another fp32 result.  (With fp32 element
arithmetic, measured: 58 of 2556 edge checks missed the bound, 55 of them with a kernel error of at most four fp32 epsilons.)"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import REL_L2_GRAD, RTOL_SCALAR, rel_l2, to_dev

gpu = pytest.mark.gpu
DEV = 'cuda:0'
NAMES = ['z', 'u_mean', 'u_tril_vec', 'log_mean', 'log_logvar']
SEED = 2.5
GRID = [(S, C, B) for S in (1, 3, 64) for C in (1, 3, 10, 37) for B in (1, 63, 512)]
P_KINDS = ['typical', 'var0', 'var1e-8', 'var25', 'y0', 'y1e4', 'm80']
T_KINDS = ['typical', 'var0', 'var1e-8', 'var25', 'resid1e3', 'ls-6', 'ls3', 'df1', 'df30']
NO_DIGIT = 0.1          # an fp32 restatement further than this (relative) from fp64 keeps no digit


# -- the fp64 yardsticks ----------------------------------------------------------------------------------------------------------
def poisson_ell(mu, var, y):
    """ell (S, C, B) in the dtype of mu; y (C, B) or (B,)."""
    y = y.to(mu.dtype)
    return y * mu - torch.exp(mu + 0.5 * var) - torch.lgamma(y + 1)


def studentt_lognorm(df):
    return math.lgamma(0.5 * (df + 1)) - math.lgamma(0.5 * df) - 0.5 * math.log(df * math.pi)


def studentt_ell(mu, var, y, log_scale, df):
    """ell (S, C, B) of the 20-node rule in the dtype of mu; y (C, B) or (B,), log_scale (C,)."""
    x, w = np.polynomial.hermite.hermgauss(20)
    x, w = torch.tensor(x, dtype=mu.dtype), torch.tensor(w / np.sqrt(np.pi), dtype=mu.dtype)
    r = y.to(mu.dtype).unsqueeze(-1) - (mu.unsqueeze(-1) + (2 * var).sqrt().unsqueeze(-1) * x)
    s2 = (2 * log_scale).exp().view(1, -1, 1, 1)
    k = studentt_lognorm(df) - log_scale.view(1, -1, 1)
    return k - 0.5 * (df + 1) * (torch.log1p(r * r / (df * s2)) * w).sum(-1)


def _shared(kind, kinds):
    """Target form of an edge kind: the (C, B) form and the shared row alternate over the kinds."""
    return kinds.index(kind) % 2 == 1


def _base(S, C, B, seed):
    gen = torch.Generator().manual_seed(seed)
    mu = torch.randn(S, C, B, generator=gen)
    var = 1e-3 + (2 - 1e-3) * torch.rand(S, C, B, generator=gen)
    return gen, mu, var


def poisson_inputs(S, C, B, kind, shared):
    """-> mu, var (S, C, B) fp32, y (C, B) or (B,)."""
    gen, mu, var = _base(S, C, B, 1000 * S + 10 * C + B)
    y = torch.poisson(torch.exp(mu[0]), generator=gen)                   # counts of the first hyper-sample's rate
    if kind == 'var0':
        var = torch.zeros_like(var)
    elif kind == 'var1e-8':
        var = torch.full_like(var, 1e-8)
    elif kind == 'var25':
        var = torch.full_like(var, 25.0)
    elif kind == 'y0':
        y = torch.zeros_like(y)
    elif kind == 'y1e4':
        y = torch.full_like(y, 1e4)
    elif kind == 'm80':
        # m = mu + var / 2 in [78, 80] at element 0 and every 1009th element (the sum of exp(m) over the largest grid shape
        # stays below the fp32 maximum), mu in [0, 60] elsewhere
        u = torch.rand(S, C, B, generator=gen)
        mu = 60 * u
        flat = mu.view(-1)
        flat[::1009] = 77 + 2 * u.view(-1)[::1009]
    return mu, var, (y[0] if shared else y)


def studentt_inputs(S, C, B, kind, shared):
    """-> mu, var (S, C, B) fp32, y (C, B) or (B,), log_scale (C,), df."""
    gen, mu, var = _base(S, C, B, 2000 * S + 10 * C + B)
    y = mu[0] + 0.3 * torch.randn(C, B, generator=gen)
    y.view(-1)[::10] += 10.0                                              # every tenth point is an outlier
    ls, df = torch.linspace(-2.5, -1.5, C), 4.0
    if kind == 'var0':
        var = torch.zeros_like(var)
    elif kind == 'var1e-8':
        var = torch.full_like(var, 1e-8)
    elif kind == 'var25':
        var = torch.full_like(var, 25.0)
    elif kind == 'resid1e3':
        sign = torch.where(torch.rand(C, B, generator=gen) < 0.5, -1.0, 1.0)
        y = mu[0] + 1e3 * sign
    elif kind == 'ls-6':
        ls = torch.full((C,), -6.0)
    elif kind == 'ls3':
        ls = torch.full((C,), 3.0)
    elif kind == 'df1':
        df = 1.0
    elif kind == 'df30':
        df = 30.0
    return mu, var, (y[0] if shared else y), ls, df


@functools.lru_cache(maxsize=None)
def poisson_ref(S, C, B, kind, shared, dtype):
    """-> (nll, sum|terms| / S, gmu, gvar, rate) of SEED * nll in `dtype` on the CPU; computed once per case and shared."""
    mu, var, y = poisson_inputs(S, C, B, kind, shared)
    m, v = (a.detach().to(dtype).clone().requires_grad_(True) for a in (mu, var))
    ell = poisson_ell(m, v, y)
    nll = -ell.mean(0).sum()
    gm, gv = torch.autograd.grad(SEED * nll, [m, v])
    return nll.item(), ell.detach().abs().sum().item() / S, gm, gv, torch.exp(m + 0.5 * v).detach()


@functools.lru_cache(maxsize=None)
def studentt_ref(S, C, B, kind, shared, dtype):
    """-> (nll, sum|terms| / S, gmu, gvar or None (var = 0), g_log_scale) of SEED * nll in `dtype` on the CPU."""
    mu, var, y, ls, df = studentt_inputs(S, C, B, kind, shared)
    m, v, l = (a.detach().to(dtype).clone().requires_grad_(True) for a in (mu, var, ls))
    with_var = kind != 'var0'
    ell = studentt_ell(m, v if with_var else v.detach(), y, l, df)
    nll = -ell.mean(0).sum()
    g = torch.autograd.grad(SEED * nll, [m, l] + ([v] if with_var else []))
    return nll.item(), ell.detach().abs().sum().item() / S, g[0], (g[2] if with_var else None), g[1]


def _errors(got, ref):
    """got / ref: (nll, scale, tensors...) -> [value error / scale, rel_l2 per tensor] (None entries dropped)."""
    out = [abs(got[0] - ref[0]) / ref[1]]
    return out + [rel_l2(a, b) for a, b in zip(got[2:], ref[2:]) if b is not None]


def _check(tag, kind, got, ref64, ref32):
    """The op-level bounds of the module docstring; prints every figure before it asserts."""
    assert all(torch.isfinite(torch.as_tensor(q)).all() for q in got if q is not None), tag
    e = _errors(got, ref64)
    if kind == 'typical':
        bound = [1e-5] * len(e)
    else:
        e32 = _errors(ref32, ref64)
        assert all(math.isfinite(q) and q < NO_DIGIT for q in e32), (tag, 'the fp32 restatement keeps no digit', e32)
        bound = [4 * q for q in e32]
    print(f'[op] {tag}: ' + ' '.join(f'{a:.2e} ({b:.2e})' for a, b in zip(e, bound)), flush=True)
    for i, (a, b) in enumerate(zip(e, bound)):
        assert a <= b, (tag, i, a, b)


# -- CPU: the restatements themselves, the factory, the routing ---------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 3, 63), (3, 10, 512)])
def test_fp32_restatement_keeps_a_digit_on_every_edge_kind(shape):
    """No edge case is left out of the accuracy table: plain fp32 torch stays within NO_DIGIT of fp64 on every quantity."""
    for kind in P_KINDS[1:]:
        sh = _shared(kind, P_KINDS)
        r64, r32 = poisson_ref(*shape, kind, sh, torch.float64), poisson_ref(*shape, kind, sh, torch.float32)
        e32 = _errors(r32, r64)
        assert all(math.isfinite(q) and q < NO_DIGIT for q in e32), ('poisson', kind, e32)
    for kind in T_KINDS[1:]:
        sh = _shared(kind, T_KINDS)
        r64, r32 = studentt_ref(*shape, kind, sh, torch.float64), studentt_ref(*shape, kind, sh, torch.float32)
        e32 = _errors(r32, r64)
        assert all(math.isfinite(q) and q < NO_DIGIT for q in e32), ('studentt', kind, e32)


class _Data:
    def __init__(self, x, y):
        self.x, self.targets = x, y

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.targets[i]


def test_create_reg_builds_each_likelihood_and_round_trips_a_state_dict():
    from vargp_amd.likelihoods import GaussianLikelihood, PoissonLikelihood, StudentTLikelihood, is_external, n_f
    from vargp_amd.vargp import VARGP
    torch.manual_seed(0)
    x = torch.randn(50, 3)
    for targets, C in ((torch.randn(50), 1), (torch.randn(50, 4), 4)):
        for name, cls in (('gaussian', GaussianLikelihood), ('studentt', StudentTLikelihood), ('poisson', PoissonLikelihood)):
            gp = VARGP.create_reg(_Data(x, targets), M=7, n_var_samples=2, likelihood=name, df=3.0)
            assert isinstance(gp.likelihood, cls) and is_external(gp.likelihood) and n_f(gp.likelihood) == 1
            assert gp.z.shape == (C, 7, 3) and gp.n_v == 2 and gp.likelihood.predict_batch_dim == -1
            sd = gp.state_dict()
            assert not any('df' in k for k in sd)
            assert ('likelihood.log_scale' in sd) == (name == 'studentt')
            if name == 'studentt':
                assert gp.likelihood.df == 3.0 and sd['likelihood.log_scale'].shape == (C,)
                assert gp.likelihood.ext_param() is gp.likelihood.log_scale
            if name == 'poisson':
                assert gp.likelihood.ext_param() is None and not any(k.startswith('likelihood') for k in sd)
            other = VARGP.create_reg(_Data(x, targets), M=7, n_var_samples=2, likelihood=name, df=3.0)
            other.load_state_dict(sd)
            for k, v in other.state_dict().items():
                assert torch.equal(v, sd[k]), k
    gp = VARGP.create_reg(_Data(x, torch.randn(50)), M=5, kernel='matern32', native_kernel=True, map_est_hypers=True)
    assert gp.kernel.nu == 1.5 and gp.kernel.map_est
    with pytest.raises(ValueError, match='create_reg'):
        VARGP.create_reg(_Data(x, torch.randn(50)), likelihood='softmax')
    with pytest.raises(ValueError, match='create_reg'):
        VARGP.create_reg(_Data(x, torch.randn(50)), kernel='linear')
    with pytest.raises(ValueError, match='create_reg'):
        VARGP.create_reg(_Data(x, torch.randn(50)), native_kernel=True)
    with pytest.raises(ValueError):
        StudentTLikelihood(2, df=0.0)


def test_create_reg_hands_the_hyper_posterior_to_the_next_task():
    from vargp_amd.vargp import VARGP
    torch.manual_seed(1)
    data = _Data(torch.randn(40, 2), torch.randn(40, 2))
    first = VARGP.create_reg(data, M=6, likelihood='studentt')
    with torch.no_grad():
        first.kernel.log_mean.add_(0.3)
        first.kernel.log_logvar.sub_(0.2)
    sd = {k: v.detach().clone() for k, v in first.state_dict().items()}
    prev = [dict(sd)]
    second = VARGP.create_reg(data, M=6, likelihood='studentt', prev_params=prev)
    assert torch.equal(second.kernel.prior_log_mean, sd['kernel.log_mean'])
    assert torch.equal(second.kernel.prior_log_logvar, sd['kernel.log_logvar'])
    assert not any(k.startswith('kernel') for k in prev[0])                 # popped, as create_clf does
    assert len(second.prev_params) == 1 and torch.equal(second.prev_params[0]['z'], sd['z'])


def test_target_forms():
    from vargp_amd import ops
    y = torch.arange(6).reshape(2, 3)
    t, ld = ops.reg_target(y, 2, 3)
    assert t.dtype == torch.float32 and ld == 3
    assert ops.reg_target(y[0], 2, 3)[1] == 0
    with pytest.raises(ValueError):
        ops.reg_target(y.t(), 2, 3)
    with pytest.raises(TypeError):
        ops.reg_target([1.0, 2.0], 1, 2)
    assert abs(ops.studentt_lognorm(1e6) + 0.5 * math.log(2 * math.pi)) < 1e-6     # -> the Gaussian constant


# -- GPU, op level ------------------------------------------------------------------------------------------------------------------
def _run_poisson(mu, var, y):
    from vargp_amd import ops
    md, vd = (a.detach().to(DEV).requires_grad_(True) for a in (mu, var))
    nll = ops.poisson_nll(md, vd, y.to(DEV))
    (SEED * nll).backward()
    return nll.detach().cpu(), md.grad.cpu(), vd.grad.cpu(), ops.poisson_predict(md.detach(), vd.detach()).cpu()


def _run_studentt(mu, var, y, ls, df):
    from vargp_amd import ops
    md, vd, ld = (a.detach().to(DEV).requires_grad_(True) for a in (mu, var, ls))
    nll = ops.studentt_nll(md, vd, y.to(DEV), ld, df)
    (SEED * nll).backward()
    return nll.detach().cpu(), md.grad.cpu(), vd.grad.cpu(), ld.grad.cpu()


@gpu
@pytest.mark.parametrize('kind', P_KINDS)
@pytest.mark.parametrize('shape', GRID, ids=lambda s: 'S%d-C%d-B%d' % s)
def test_poisson_op_vs_fp64(shape, kind):
    S, C, B = shape
    for shared in ((False, True) if kind == 'typical' else (_shared(kind, P_KINDS),)):
        mu, var, y = poisson_inputs(S, C, B, kind, shared)
        a, b = _run_poisson(mu, var, y), _run_poisson(mu, var, y)
        for p, q in zip(a, b):                              # no float atomics: bitwise reproducible
            assert torch.equal(p, q)
        assert a[3].shape == (S, C, B)
        r64 = poisson_ref(S, C, B, kind, shared, torch.float64)
        r32 = None if kind == 'typical' else poisson_ref(S, C, B, kind, shared, torch.float32)
        _check(f'poisson S{S} C{C} B{B} {kind} {"shared" if shared else "full"} (value gmu gvar rate)', kind,
               (a[0].item(), None) + a[1:], r64, r32)


@gpu
@pytest.mark.parametrize('kind', T_KINDS)
@pytest.mark.parametrize('shape', GRID, ids=lambda s: 'S%d-C%d-B%d' % s)
def test_studentt_op_vs_fp64(shape, kind):
    S, C, B = shape
    for shared in ((False, True) if kind == 'typical' else (_shared(kind, T_KINDS),)):
        mu, var, y, ls, df = studentt_inputs(S, C, B, kind, shared)
        a, b = _run_studentt(mu, var, y, ls, df), _run_studentt(mu, var, y, ls, df)
        for p, q in zip(a, b):
            assert torch.equal(p, q)
        if kind == 'var0':
            assert torch.count_nonzero(a[2]) == 0           # the rule's variance gradient at var = 0: exactly 0
        r64 = studentt_ref(S, C, B, kind, shared, torch.float64)
        r32 = None if kind == 'typical' else studentt_ref(S, C, B, kind, shared, torch.float32)
        _check(f'studentt S{S} C{C} B{B} {kind} {"shared" if shared else "full"} (value gmu gvar g_log_scale)', kind,
               (a[0].item(), None) + a[1:], r64, r32)


@gpu
@pytest.mark.parametrize('shape', [(3, 10, 512), (64, 37, 512), (1, 1, 1), (2, 5, 63)])
def test_bwd_writes_the_forward_value(shape):
    """The trainer's single call (bwd with nll) leaves exactly the forward's value; every entry is bitwise reproducible."""
    from vargp_amd import ops
    S, C, B = shape
    seed = torch.tensor([3.0], device=DEV)
    for shared in (False, True):
        mu, var, y = (a.to(DEV) for a in poisson_inputs(S, C, B, 'var25', shared))
        tgt = ops.reg_target(y, C, B)
        out = []
        for _ in range(2):
            a, b = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
            gmu, gvar = torch.empty_like(mu), torch.empty_like(var)
            ops.lik_nll_fwd('poisson', mu, var, tgt, (), a)
            ops.lik_nll_bwd('poisson', mu, var, tgt, (), seed, gmu, gvar, nll=b)
            assert torch.equal(a, b) and torch.isfinite(a).all()
            out.append((a, gmu, gvar, ops.poisson_predict(mu, var)))
        assert all(torch.equal(p, q) for p, q in zip(*out))
        mu, var, y, ls, df = studentt_inputs(S, C, B, 'typical', shared)
        mu, var, y, ls = (a.to(DEV) for a in (mu, var, y, ls))
        tgt = ops.reg_target(y, C, B)
        out = []
        for _ in range(2):
            a, b = torch.empty(1, device=DEV), torch.empty(1, device=DEV)
            gmu, gvar, gls = torch.empty_like(mu), torch.empty_like(var), torch.empty_like(ls)
            extra = (ls, df, ops.studentt_lognorm(df))
            ops.lik_nll_fwd('studentt', mu, var, tgt, extra, a)
            ops.lik_nll_bwd('studentt', mu, var, tgt, extra, seed, gmu, gvar, gls, nll=b)
            assert torch.equal(a, b) and torch.isfinite(a).all()
            out.append((a, gmu, gvar, gls))
        assert all(torch.equal(p, q) for p, q in zip(*out))


@gpu
def test_c_abi_argument_checks():
    from vargp_amd._lib import lib, ptr, stream_ptr
    mu, var = torch.zeros(2, 3, 4, device=DEV), torch.ones(2, 3, 4, device=DEV)
    y, ls = torch.zeros(3, 4, device=DEV), torch.zeros(3, device=DEV)
    out, ws = torch.zeros(1, device=DEV), torch.zeros(64, device=DEV)
    pois = lambda y_, ldy=4, wsb=256: lib().vargp_poisson_nll_fwd(ptr(mu), ptr(var), ptr(y_), ldy, ptr(out), 2, 3, 4, ptr(ws), wsb,
                                                                  stream_ptr())
    assert pois(y) == 0 and pois(y, ldy=0) == 0
    assert pois(None) != 0 and pois(y, ldy=3) != 0 and pois(y, wsb=0) != 0
    stud = lambda ls_, df, wsb=256: lib().vargp_studentt_nll_fwd(ptr(mu), ptr(var), ptr(y), 4, ptr(ls_), df, 0.0, ptr(out), 2, 3, 4,
                                                                ptr(ws), wsb, stream_ptr())
    assert stud(ls, 4.0) == 0
    assert stud(None, 4.0) != 0 and stud(ls, 0.0) != 0 and stud(ls, -1.0) != 0 and stud(ls, 4.0, wsb=8) != 0
    assert lib().vargp_poisson_workspace_bytes(3, 10, 512) == 10 * 6 * 8
    assert lib().vargp_studentt_workspace_bytes(3, 10, 512) == 2 * 10 * 6 * 8
    assert lib().vargp_studentt_workspace_bytes(64, 37, 512) == 2 * 37 * 32 * 8
    torch.cuda.synchronize()


# -- GPU, model level: the native program route against the composed per-op route of the same model -----------------------------
def _make_lik(name, C):
    from vargp_amd.likelihoods import GaussianLikelihood, PoissonLikelihood, StudentTLikelihood
    if name == 'poisson':
        return PoissonLikelihood()
    if name == 'gaussian':
        return GaussianLikelihood(C)
    lik = StudentTLikelihood(C, df=4.0)
    with torch.no_grad():
        lik.log_scale.copy_(torch.linspace(-1.5, -0.5, C))
    return lik


def _build(params, prev, S, name, kernel='rbf', cls=None):
    from vargp_amd.kernels import MaternKernel, RBFKernel
    from vargp_amd.vargp import VARGP
    C, D = params['z'].shape[0], params['z'].shape[-1]
    kw = dict(prior_log_mean=params['prior_log_mean'], prior_log_logvar=params['prior_log_logvar'])
    kern = RBFKernel(D, **kw) if kernel == 'rbf' else MaternKernel(D, nu=kernel, native=True, **kw)
    pp = [{k: v.clone() for k, v in p.items()} for p in prev]
    if cls is not None:
        gp = cls(params['z'], kern, _make_lik(name, C), n_var_samples=S, prev_params=to_dev(pp, DEV))
    else:
        gp = VARGP(params['z'], kern, _make_lik(name, C), n_var_samples=S, prev_params=pp)
    with torch.no_grad():
        gp.kernel.log_mean.copy_(params['log_mean'])
        gp.kernel.log_logvar.copy_(params['log_logvar'])
        gp.u_mean.copy_(params['u_mean'])
        gp.u_tril_vec.copy_(params['u_tril_vec'])
    return gp.to(DEV)


def _grads(gp):
    g = dict(z=gp.z.grad, u_mean=gp.u_mean.grad, u_tril_vec=gp.u_tril_vec.grad, log_mean=gp.kernel.log_mean.grad,
             log_logvar=gp.kernel.log_logvar.grad)
    if gp.likelihood.ext_param() is not None:
        g['log_scale'] = gp.likelihood.log_scale.grad
    return g


def _targets(name, C, B, seed, shared=False):
    gen = torch.Generator().manual_seed(seed)
    if name == 'poisson':
        y = torch.poisson(torch.exp(0.7 * torch.randn(C, B, generator=gen)), generator=gen)
    else:
        y = 0.6 * torch.randn(C, B, generator=gen)
        y.view(-1)[::10] += 10.0
    return y[0] if shared else y


def _problem(shape, seed):
    S, C, M, D, B, n_prev = shape
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=seed, kind='gauss')
    return params, prev, x, {k: v for k, v in nz.items() if k != 'eps_f'}


# (S, C, M, D, B, n_prev), kernel, shared targets -> the program expected
MODEL_CASES = [
    ((2, 5, 24, 16, 48, 0), 'rbf', False, 't0'),       # first-task program, direct distances
    ((3, 3, 12, 4, 40, 1), 'rbf', True, 'tn'),         # block program, direct distances
    ((1, 7, 20, 36, 70, 1), 'rbf', False, 'tn'),       # block program, MFMA distances
    ((2, 3, 56, 40, 64, 0), 'rbf', False, 't0'),       # first-task program (csrc/elbo_t0.hip), D = 40
    ((2, 3, 12, 8, 40, 1), 1.5, False, 'tn'),          # MaternKernel(native=True)
]


@gpu
@pytest.mark.parametrize('name', ['poisson', 'studentt'])
@pytest.mark.parametrize('case', MODEL_CASES, ids=lambda c: '-'.join(str(v) for v in c[0]) + f'-{c[1]}')
def test_program_route_vs_composed_route(case, name):
    from vargp_amd import noise
    shape, kernel, shared, expect = case
    S, C, M, D, B, n_prev = shape
    seed = 17 * S + 5 * C + M + D + B + n_prev
    params, prev, x, nz = _problem(shape, seed)
    y = _targets(name, C, B, seed, shared)
    beta, scale = 2.0, 10.0
    res = []
    for composed in (True, False):
        gp = _build(params, prev, S, name, kernel)
        if composed:
            gp.fused_first_task = gp.fused_tasks = False
        with noise.inject(**to_dev(nz, DEV)):
            kh, ku, nl = gp.loss(x.to(DEV), y.to(DEV))
            (beta * kh + ku + scale * nl).backward()
        on = (bool(gp._t0_progs), bool(gp._tn_progs))
        assert on == ((False, False) if composed else (expect == 't0', expect == 'tn')), (composed, on)
        if not composed and kernel != 'rbf':
            assert all(p.kernel_nu2 == 3 for p in gp._tn_progs.values())
        res.append(([kh.item(), ku.item(), nl.item()], {k: v.detach().cpu().clone() for k, v in _grads(gp).items()}))
    (sc_c, g_c), (sc_p, g_p) = res
    assert all(math.isfinite(v) for v in sc_p)
    for a, b, k in zip(sc_p, sc_c, ['kl_hypers', 'kl_u', 'nll']):
        np.testing.assert_allclose(a, b, rtol=RTOL_SCALAR, err_msg=k)
    assert set(g_p) == set(NAMES) | ({'log_scale'} if name == 'studentt' else set())
    for k in g_p:
        assert rel_l2(g_p[k], g_c[k]) < REL_L2_GRAD, k


# -- GPU, trainer -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('name', ['poisson', 'studentt'])
@pytest.mark.parametrize('n_prev', [0, 1])
def test_trainer_graph_step_equals_eager_step(n_prev, name):
    from vargp_amd import noise, ops
    from vargp_amd.train import ElboTrainer
    S, C, M, D, B = 3, 4, 20, 2, 100
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=303 + n_prev, kind='wtoy')
    nz = {k: v for k, v in nz.items() if k != 'eps_f'}
    xd, yd = x.to(DEV), _targets(name, C, B, 5).to(DEV)
    ops.set_cholesky_error_mode('defer')
    ops.reset_linalg_errors()
    try:
        results = []
        for mode in ('eager', 'graph'):
            gp = _build(params, prev, S, name)
            tr = ElboTrainer(gp, lr=1e-3, beta=1.0, n_total=float(B))
            assert tr._t0 and tr.ext
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
        assert ('likelihood.log_scale' in sd_e) == (name == 'studentt')
        if name == 'studentt':                                 # the likelihood's own parameter is trained by the step
            assert not torch.equal(sd_e['likelihood.log_scale'], torch.linspace(-1.5, -0.5, C))
        assert ops.linalg_error_count() == 0
    finally:
        ops.set_cholesky_error_mode('raise')


@gpu
@pytest.mark.parametrize('name', ['poisson', 'studentt'])
@pytest.mark.parametrize('shape', [(2, 5, 24, 16, 48, 0), (3, 3, 12, 4, 40, 1)])
def test_retained_graph_second_backward_doubles_the_gradient(shape, name):
    from vargp_amd import noise
    S, C, M, D, B, n_prev = shape
    params, prev, x, nz = _problem(shape, 77)
    y = _targets(name, C, B, 77)
    res = []
    for twice in (False, True):
        gp = _build(params, prev, S, name)
        with noise.inject(**to_dev(nz, DEV)):
            kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
        loss = 2.0 * kl_h + kl_u + 3.0 * nll
        if twice:
            loss.backward(retain_graph=True)
        loss.backward()
        res.append({k: v.detach().cpu().clone() for k, v in _grads(gp).items()})
    assert ('log_scale' in res[0]) == (name == 'studentt')
    for k in res[0]:
        assert rel_l2(res[1][k], 2 * res[0][k]) < 1e-5, k


# -- GPU, predict -------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('n_prev,D', [(0, 8), (1, 40)])
@pytest.mark.parametrize('name', ['poisson', 'studentt'])
def test_predict_shape_and_tiled_sweep(n_prev, D, name):
    from vargp_amd import noise
    S, C, M, B = 2, 3, 12, 100
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=n_prev, seed=41 + n_prev, kind='gauss')
    gp = _build(params, prev, S, name)
    xd = x.to(DEV)
    with noise.inject(eps_theta=nz['eps_theta'].to(DEV)), torch.no_grad():
        one = gp.predict(xd)
        tiled = gp.predict(xd, tile=32)
        mu, var = gp(xd)
    assert one.shape == (S, C, B) and tiled.shape == (S, C, B)
    want = torch.exp(mu.double() + 0.5 * var.double()) if name == 'poisson' else mu.double()
    np.testing.assert_allclose(one.cpu().numpy(), want.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(tiled.cpu().numpy(), one.cpu().numpy(), rtol=1e-4, atol=1e-4)


@gpu
@pytest.mark.parametrize('name', ['poisson', 'studentt', 'gaussian'])
def test_retrain_model_tiled_predict_joins_along_the_batch(name):
    """VARGPRetrain.predict(tile=) joins its chunks along the likelihood's batch dim ((S, C, B): the last)."""
    from vargp_amd import noise
    from vargp_amd.vargp_retrain import VARGPRetrain
    S, C, M, D, B = 2, 3, 12, 2, 64
    params, prev, x, _, nz = orc.make_problem(S, 1, C, M, D, B, n_prev=1, seed=308, kind='wtoy')
    gp = _build(params, prev, S, name, cls=VARGPRetrain)
    with noise.inject(eps_theta=nz['eps_theta'].to(DEV)), torch.no_grad():
        one, tiled = gp.predict(x.to(DEV)), gp.predict(x.to(DEV), tile=24)
    assert one.shape == (S, C, B) and tiled.shape == (S, C, B)
    np.testing.assert_allclose(tiled.cpu().numpy(), one.cpu().numpy(), rtol=1e-4, atol=1e-4)


# -- GPU, refusals: what a Gaussian model is refused, these are refused, in the same words ------------------------------------------
@gpu
@pytest.mark.parametrize('name,cls_name', [('poisson', 'PoissonLikelihood'), ('studentt', 'StudentTLikelihood')])
def test_routes_that_assume_the_softmax_refuse_these_models(name, cls_name, tmp_path):
    import torch.distributed as dist
    from vargp_amd import ops
    from vargp_amd.train import ElboTrainer
    S, C, M, D, B = 3, 4, 20, 2, 100
    params, prev, x, _, _ = orc.make_problem(S, 1, C, M, D, B, n_prev=0, seed=301, kind='wtoy')
    xd, yd = x.to(DEV), _targets(name, C, B, 1).to(DEV)
    gp = _build(params, prev, S, name)
    assert not gp._lazy_ok()                       # the lazy route: the node route instead
    kl_h, _, _ = gp.loss(xd, yd)
    assert torch.is_tensor(kl_h) and kl_h.grad_fn is not None
    with pytest.raises(NotImplementedError, match=cls_name):
        gp.elbo_tiled(xd, yd, tile=50)
    ops.set_cholesky_error_mode('defer')
    try:
        tr = ElboTrainer(gp, lr=1e-3)
        tr.capture(xd, yd, warmup=1)
        with pytest.raises(NotImplementedError, match=cls_name):
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
            ElboTrainer(_build(params, prev, S, name), force_exchange=True)
        with pytest.raises(NotImplementedError):
            ElboTrainer(_build(params, prev, S, name), force_exchange=True, shards=[(0, 3, 0, 4)])
    finally:
        if own:
            dist.destroy_process_group()


# -- GPU, behaviour -----------------------------------------------------------------------------------------------------------------
def _train(gp, x, y, steps, seed):
    """`steps` eager trainer steps on minibatches of 64; y (N,) (one output)."""
    from vargp_amd.train import ElboTrainer
    N = x.shape[0]
    tr = ElboTrainer(gp, lr=3e-2, beta=1.0, n_total=N, noise_seed=seed)
    xd, yd = x.to(DEV), y.to(DEV)
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        idx = torch.randint(0, N, (64,), generator=gen).to(DEV)
        out = tr.step(xd[idx], yd[idx])
    assert all(torch.isfinite(o).item() for o in out)


@gpu
def test_student_t_model_resists_outliers_better_than_the_gaussian_model():
    """1-D function, 300 points, 5 % of the targets shifted by +8, 400 trainer steps: the StudentTLikelihood(df=4) model's RMSE to
    the clean function is below the GaussianLikelihood model's on the same data and seed.  The ordering only, no threshold.
    Measured: see the table there."""
    from vargp_amd.vargp import VARGP
    f = lambda x: torch.sin(2 * x[:, 0]) + 0.5 * x[:, 0]
    gen = torch.Generator().manual_seed(0)
    x = 4 * torch.rand(300, 1, generator=gen) - 2
    y = f(x) + 0.1 * torch.randn(300, generator=gen)
    y[torch.randperm(300, generator=gen)[:15]] += 8.0
    xt = torch.linspace(-2, 2, 200).unsqueeze(-1)
    rmse = {}
    for name in ('studentt', 'gaussian'):
        torch.manual_seed(0)
        gp = VARGP.create_reg(_Data(x, y), M=20, n_var_samples=3, likelihood=name, df=4.0).to(DEV)
        _train(gp, x, y, 400, seed=11)
        with torch.no_grad():
            pred = gp.predict(xt.to(DEV)).mean(0)[0].cpu()
        rmse[name] = (pred - f(xt)).pow(2).mean().sqrt().item()
    print(f'[behaviour] RMSE to the clean function: studentt {rmse["studentt"]:.4f}, gaussian {rmse["gaussian"]:.4f}', flush=True)
    assert rmse['studentt'] < rmse['gaussian'], rmse


@gpu
def test_poisson_model_learns_the_rate():
    """Counts drawn from exp(f) for a smooth f: the predicted rate's mean absolute error on 500 held-out points drops by at least
    half from initialisation to step 400."""
    from vargp_amd.vargp import VARGP
    f = lambda x: 1.0 + torch.sin(2 * x[:, 0])
    gen = torch.Generator().manual_seed(1)
    x = 4 * torch.rand(600, 1, generator=gen) - 2
    y = torch.poisson(torch.exp(f(x)), generator=gen)
    xt = 4 * torch.rand(500, 1, generator=gen) - 2
    torch.manual_seed(1)
    gp = VARGP.create_reg(_Data(x, y), M=20, n_var_samples=3, likelihood='poisson').to(DEV)

    def mae():
        with torch.no_grad():
            return (gp.predict(xt.to(DEV)).mean(0)[0].cpu() - torch.exp(f(xt))).abs().mean().item()
    before = mae()
    _train(gp, x, y, 400, seed=13)
    after = mae()
    print(f'[behaviour] Poisson rate MAE on 500 held-out points: {before:.4f} at initialisation, {after:.4f} at step 400', flush=True)
    assert after <= 0.5 * before, (before, after)
