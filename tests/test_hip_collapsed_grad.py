"""The differentiable collapsed bound on the device: ops.gram_moments_diff and its fused backward (csrc/moments.hip:
vargp_gram_moments_bwd), VARGP.collapsed_bound, VARGP.fit_collapsed_ and create_reg(q_init='collapsed'), against the fp64
restatements of tests/test_collapsed.py and tests/test_collapsed_grad.py.

Rule (tests/sweep_rule.py): device error against fp64 <= tolerance + 2 x the error of the fp32 restatement on one host thread.
REL_L2_GRAD (relative L2) for gZ (per output), gtheta[:D] and the bound's gradients; RTOL_SCALAR for gtheta[D] and the bound."""
import math

import pytest
import torch

from helpers import REL_L2_GRAD, RTOL_SCALAR, rel_l2
from test_collapsed import _Data, ref_moments, ref_vec2tril
from test_collapsed_grad import TOY_KERNEL, TOY_LENGTHSCALE, TOY_START, ref_bound_grads, toy_regression
from test_hip_collapsed import _chain, _moment_problem, _one_thread

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# (Mt, N, D, G, nu2, weights): one, two and three 64-row panels, both sides of the 64-column step, several chunks, both sides of
# kRbfDirectD = 32, and D = 784, which takes two groups of d per panel
GRAD_CASES = [
    (1, 1, 1, 1, 0, None), (15, 63, 2, 3, 1, 'rand'), (64, 64, 32, 1, 3, 'zeros'), (65, 65, 33, 3, 5, None),
    (130, 1000, 40, 1, 0, 'rand'), (15, 1000, 2, 1, 0, 'zeros'), (130, 1000, 1, 3, 3, 'rand'), (33, 1000, 33, 1, 1, 'zeros'),
    (100, 300, 784, 2, 0, 'rand'), (130, 1, 2, 1, 5, None),
]


def _grad_problem(Mt, N, D, G, wmode, seed):
    theta, Z, X, w, y, keep = _moment_problem(Mt, N, D, G, wmode, seed)
    if D == 784:
        X, Z = 0.12 * X, 0.12 * Z
    g = torch.Generator().manual_seed(seed + 1)
    return theta, Z, X, w, y, keep, torch.randn(G, Mt, Mt, generator=g), torch.randn(G, Mt, generator=g)


def _ref_grads(theta, Z, X, w, y, gPhi, gc, nu2, dtype):
    """autograd of ref_moments under <gPhi, Phi> + <gc, c>, output by output (the dense route holds a (Mt, N, D) tensor)"""
    th = theta.to(dtype).clone().requires_grad_(True)
    Zr = Z.to(dtype).clone().requires_grad_(True)
    for g in range(Z.shape[0]):
        Phi, c, _ = ref_moments(th, Zr[g:g + 1], X, None if w is None else w[g:g + 1], y[g:g + 1], nu2, dtype=dtype)
        ((gPhi[g:g + 1].to(dtype) * Phi).sum() + (gc[g:g + 1].to(dtype) * c).sum()).backward()
    return Zr.grad, th.grad


def _dev_grads(theta, Z, X, w, y, gPhi, gc, nu2):
    """the same through ops.gram_moments_diff; -> gZ, gtheta on the host"""
    from vargp_amd import ops
    dev = lambda t: None if t is None else t.to(DEV)
    th, Zd = dev(theta).requires_grad_(True), dev(Z).requires_grad_(True)
    Phi, c, sums = ops.gram_moments_diff(th, Zd, dev(X), dev(w), dev(y), nu2)
    assert not sums.requires_grad
    ((dev(gPhi) * Phi).sum() + (dev(gc) * c).sum()).backward()
    return Zd.grad.cpu(), th.grad.cpu()


def _hold_to_rule(got, r32, r64, tag):
    (gZ, gth), (gZ32, gth32), (gZ64, gth64) = got, r32, r64
    D = gth.numel() - 1
    errs = [(f'gZ[{g}]', rel_l2(gZ[g], gZ64[g]), rel_l2(gZ32[g], gZ64[g])) for g in range(gZ.shape[0])]
    errs.append(('gtheta[:D]', rel_l2(gth[:D], gth64[:D]), rel_l2(gth32[:D], gth64[:D])))
    for name, e, e32 in errs:
        print(f'{tag} {name}: err {e:.2e} (fp32 host {e32:.2e})')
        assert e <= REL_L2_GRAD + 2.0 * e32, (tag, name, e, e32)
    den = abs(gth64[D].item())
    e, e32 = abs(gth[D].item() - gth64[D].item()) / den, abs(gth32[D].item() - gth64[D].item()) / den
    print(f'{tag} gtheta[D]: err {e:.2e} (fp32 host {e32:.2e})')
    assert e <= RTOL_SCALAR + 2.0 * e32, (tag, e, e32)


@pytest.mark.parametrize('Mt,N,D,G,nu2,wmode', GRAD_CASES, ids=['-'.join(map(str, c)) for c in GRAD_CASES])
def test_moment_gradients_against_fp64(Mt, N, D, G, nu2, wmode):
    from vargp_amd import ops
    theta, Z, X, w, y, keep, gPhi, gc = _grad_problem(Mt, N, D, G, wmode, seed=Mt + 7 * N + 13 * D)
    assert not torch.equal(gPhi, gPhi.mT) or Mt == 1
    got = _dev_grads(theta, Z, X, w, y, gPhi, gc, nu2)
    assert got[0].shape == Z.shape and got[1].shape == theta.shape
    assert all(t.dtype == torch.float32 and bool(torch.isfinite(t).all()) for t in got)
    junk = torch.full((1 << 20,), float('nan'), device=DEV)                         # (the pooled scratch is reused: poison what follows it)
    again = _dev_grads(theta, Z, X, w, y, gPhi, gc, nu2)
    del junk
    assert all(torch.equal(u, v) for u, v in zip(got, again))                       # two calls are bitwise equal
    r64 = _ref_grads(theta, Z, X, w, y, gPhi, gc, nu2, torch.float64)
    r32 = _one_thread(lambda: _ref_grads(theta, Z, X, w, y, gPhi, gc, nu2, torch.float32))
    tag = f'Mt{Mt} N{N} D{D} G{G} nu2={nu2} w={wmode}'
    _hold_to_rule(got, r32, r64, tag)
    if wmode == 'zeros' and keep >= 1:
        # the zero-weight points removed.  One chunk on both sides: the kept points sit in the same columns of the same steps and a
        # zero weight gives V = +-0 exactly: bitwise equal (gtheta[D] comes from the forward's outputs, bitwise equal as well)
        cut = _dev_grads(theta, Z, X[:keep], w[:, :keep], y[:, :keep], gPhi, gc, nu2)
        if ops.gram_moments_bwd_chunks(G, Mt, N, D) == 1 and ops.gram_moments_bwd_chunks(G, Mt, keep, D) == 1 \
                and ops.gram_moments_chunks(G, Mt, N, D) == 1 and ops.gram_moments_chunks(G, Mt, keep, D) == 1:
            assert all(torch.equal(u, v) for u, v in zip(got, cut)), tag
        else:
            _hold_to_rule(cut, r32, r64, tag + ' (removed)')


def test_multi_chunk_and_bitwise_cases_are_covered():
    from vargp_amd import ops
    multi = [c for c in GRAD_CASES if ops.gram_moments_bwd_chunks(c[3], c[0], c[1], c[2]) > 1]
    assert multi and any(c[2] <= 32 for c in multi) and any(c[2] > 32 for c in multi), multi
    one = [c for c in GRAD_CASES if c[5] == 'zeros' and ops.gram_moments_bwd_chunks(c[3], c[0], c[1], c[2]) == 1]
    assert one, 'no zero-weight case is held to bitwise equality'


def test_padding_columns_are_masked_not_weighted():
    """N = 70 points at the head of a buffer whose next rows are NaN, in a 128-column chunk: nothing behind row N is used."""
    from vargp_amd import ops
    for D, nu2 in ((5, 0), (40, 3)):
        theta, Z, X, w, y, _, gPhi, gc = _grad_problem(33, 70, D, 2, 'rand', seed=5)
        assert ops.gram_moments_bwd_chunks(2, 33, 70, D) == 1
        Xbig = torch.full((256, D), float('nan'))
        Xbig[:70] = X
        dev = lambda t: t.to(DEV)
        a = ops.gram_moments_bwd(dev(theta), dev(Z), dev(X), dev(w), dev(y), dev(gPhi), dev(gc), nu2)
        b = ops.gram_moments_bwd(dev(theta), dev(Z), dev(Xbig)[:70], dev(w), dev(y), dev(gPhi), dev(gc), nu2)
        for u, v in zip(a, b):
            u, v = (u, v) if u.dim() == 3 else (u[:D], v[:D])                       # (entry D of gtheta is the caller's)
            assert torch.equal(u, v) and bool(torch.isfinite(u).all())


@pytest.mark.parametrize('D', [2, 40])
@pytest.mark.parametrize('nu2', [0, 3, 5])
def test_coincident_points(nu2, D):
    """Every second row of Z is a row of X (d2 = 0 there).  fp64 autograd of sqrt(d2) is no yardstick at d2 = 0, so the fused
    backward is compared with the composed route on the device -- the gram op's K, Phi and c by torch, .backward() -- whose own
    error against fp64 is measured on the rows of Z that coincide with nothing."""
    from vargp_amd import ops
    Mt, N, G = 40, 150, 2
    theta, Z, X, w, y, _, gPhi, gc = _grad_problem(Mt, N, D, G, 'rand', seed=11 + nu2 + D)
    Z[:, ::2] = X[:2 * Mt:4]
    free = torch.arange(1, Mt, 2)
    got = _dev_grads(theta, Z, X, w, y, gPhi, gc, nu2)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    dev = lambda t: t.to(DEV)
    th, Zd = dev(theta).requires_grad_(True), dev(Z).requires_grad_(True)
    gram = ops.rbf_gram if nu2 == 0 else (lambda *a: ops.matern_gram(*a, nu=nu2 / 2))
    K = gram(th.view(1, -1), Zd, dev(X), True)[0]                                   # (G, Mt, N)
    Phi = (K * dev(w).unsqueeze(-2)) @ K.mT
    c = (K * dev(w * y).unsqueeze(-2)).sum(-1)
    ((dev(gPhi) * Phi).sum() + (dev(gc) * c).sum()).backward()
    cZ, cth = Zd.grad.cpu(), th.grad.cpu()
    gZ64, _ = _ref_grads(theta, Z, X, w, y, gPhi, gc, nu2, torch.float64)
    assert bool(torch.isfinite(gZ64[:, free]).all())
    own = rel_l2(cZ[:, free], gZ64[:, free])
    for name, a, b in (('gZ', got[0], cZ), ('gtheta', got[1], cth)):
        e = rel_l2(a, b)
        print(f'nu2={nu2} D{D} {name}: fused against composed {e:.2e} (composed against fp64 on the free rows {own:.2e})')
        assert e <= REL_L2_GRAD + 2.0 * own, (nu2, D, name, e, own)
    assert rel_l2(got[0][:, free], gZ64[:, free]) <= REL_L2_GRAD + 2.0 * own


# -- the bound ----------------------------------------------------------------------------------------------------------------------
BOUND_CASES = [(C, M, t, k, D) for (C, M, t) in ((1, 15, 0), (3, 33, 2)) for k in ('rbf', 'matern32') for D in (2, 40)]


@pytest.mark.parametrize('C,M,n_prev,kernel,D', BOUND_CASES, ids=['-'.join(map(str, c)) for c in BOUND_CASES])
def test_collapsed_bound_and_its_gradients(C, M, n_prev, kernel, D):
    gp, data = _chain(C, M, n_prev, kernel, D)
    x = data.x.to(DEV)
    y = (data.targets if C == 1 else data.targets.t().contiguous()).to(DEV)
    params = (gp.z, gp.kernel.log_mean, gp.likelihood.obs_log_var)
    bound = gp.collapsed_bound(x, y)
    assert bound.shape == (C,) and bound.dtype == torch.float64 and bound.requires_grad
    grads = [g.cpu() for g in torch.autograd.grad(bound.sum(), params)]
    assert all(p.grad is None for p in gp.parameters())
    for p in gp.prev_params:                                                        # the frozen tasks are constants
        assert all(not t.requires_grad and t.grad is None for t in p.values() if isinstance(t, torch.Tensor))
    nu2 = int(round(2 * gp.kernel.nu)) if hasattr(gp.kernel, 'nu') else 0
    prev = lambda dt: [dict(z=p['z'].cpu(), u_mean=p['u_mean'].cpu(), u_tril=ref_vec2tril(p['u_tril_vec'].cpu().to(dt), M))
                       for p in gp.prev_params]
    z_lt = torch.cat([p['z'].cpu() for p in gp.prev_params], -2) if n_prev else torch.zeros(C, 0, D)
    yh = (data.targets.unsqueeze(0) if C == 1 else data.targets.t()).contiguous()
    restate = lambda dt: ref_bound_grads(gp.kernel.log_mean.detach().cpu(), z_lt, gp.z.detach().cpu(), prev(dt), data.x, yh, None,
                                         gp.likelihood.obs_log_var.detach().cpu(), nu2, dtype=dt)
    (b64, (gth64, gz64, go64)), (b32, (gth32, gz32, go32)) = restate(torch.float64), _one_thread(lambda: restate(torch.float32))
    tag = f'C{C} M{M} t{n_prev} {kernel} D{D}'
    rel = lambda a, b: ((a.double() - b).abs() / b.abs()).max().item()
    e32 = rel(b32, b64)
    fit = gp.fit_q_(x, y)
    e, ef = rel(bound.detach().cpu(), b64), rel(bound.detach().cpu(), fit.bound.cpu())
    # the value is fit_q_'s (how close that is to fp64 is tests/test_hip_collapsed.py's subject; printed here)
    print(f'{tag} bound {bound.tolist()}: against fit_q_ {ef:.2e}; against fp64 {e:.2e} (fp32 host {e32:.2e})')
    assert ef <= RTOL_SCALAR + 2.0 * e32, (tag, ef, e32)
    bad = []
    for name, g, g32, g64 in (('z', grads[0], gz32, gz64), ('log_mean', grads[1], gth32, gth64), ('obs_log_var', grads[2], go32, go64)):
        e, e32 = rel_l2(g, g64), rel_l2(g32, g64)
        print(f'{tag} grad {name}: err {e:.2e} (fp32 host {e32:.2e})')
        if not (g.shape == g64.shape and e <= REL_L2_GRAD + 2.0 * e32):
            bad.append((name, e, e32))
    assert not bad, (tag, bad)


def _toy_model(x, y):
    from vargp_amd.vargp import VARGP
    torch.manual_seed(1)
    gp = VARGP.create_reg(_Data(x.cpu(), y.cpu()), M=10, map_est_hypers=True, kernel=TOY_KERNEL)
    with torch.no_grad():
        gp.kernel.log_mean.copy_(torch.tensor([math.log(TOY_START * TOY_LENGTHSCALE), 0.0]))
    return gp.to(DEV)


def test_fit_collapsed_beats_fit_q_alone_from_a_bad_lengthscale():
    """The 1-D toy of tests/test_collapsed_grad.py (N = 400, M = 10, Matern-1/2, lengthscale 10 times too long), 60 steps."""
    x, y, xs, ys = [t.to(DEV) for t in toy_regression()]
    alone, moved = _toy_model(x, y), _toy_model(x, y)
    alone.fit_q_(x, y)
    z0 = moved.z.detach().clone()
    trace = moved.fit_collapsed_(x, y, n_steps=60, lr=0.05)
    assert trace.shape == (61, 1) and trace.dtype == torch.float64 and trace.device.type == 'cpu'
    assert bool(torch.isfinite(trace).all()) and trace[-1, 0] > trace[0, 0]
    assert not torch.equal(z0, moved.z.detach()) and all(p.grad is None for p in moved.parameters())
    again = moved.fit_q_(x, y).bound.cpu()
    assert abs(trace[-1, 0].item() - again[0].item()) <= RTOL_SCALAR * abs(again[0].item())
    lp_alone, lp_moved = alone.log_prob(xs, ys).sum().item(), moved.log_prob(xs, ys).sum().item()
    print(f'bound {trace[0, 0].item():.1f} -> {trace[-1, 0].item():.1f}; held-out log density {lp_alone:.1f} (fit_q_ alone) -> '
          f'{lp_moved:.1f}; lengthscale {moved.kernel.log_mean[0].exp().item():.3f}')
    assert lp_moved > lp_alone
    # a subset of the parameters: the others stay bitwise where they were
    kept = _toy_model(x, y)
    before = [p.detach().clone() for p in (kept.z, kept.likelihood.obs_log_var, kept.kernel.log_mean)]
    kept.fit_collapsed_(x, y, n_steps=2, params=('kernel',))
    assert torch.equal(before[0], kept.z.detach()) and torch.equal(before[1], kept.likelihood.obs_log_var.detach())
    assert not torch.equal(before[2], kept.kernel.log_mean.detach())


def test_q_init_collapsed_is_create_reg_then_fit_collapsed():
    from vargp_amd.vargp import VARGP
    gp0, data = _chain(2, 5, 0, 'rbf', 3)
    made = []
    for q_init in ('default', 'collapsed'):
        torch.manual_seed(9)
        gp = VARGP.create_reg(data, M=5, q_init=q_init, collapsed_steps=3)
        assert gp.z.device == data.x.device                                         # back where the default route leaves it
        made.append(gp.to(DEV))
    made[0].fit_collapsed_(data.x.to(DEV), data.targets.t().contiguous().to(DEV), n_steps=3)
    a, b = made[0].state_dict(), made[1].state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
