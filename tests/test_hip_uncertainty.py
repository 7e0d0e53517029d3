"""Predictive entropy split into noise and knowledge (csrc/uncertainty.hip, ops.softmax_uncertainty / bernoulli_uncertainty,
likelihood.uncertainty, VARGP.uncertainty, train_utils.compute_uncertainty, the driver's --uncertainty).  Not in the reference, so
the yardstick is the fp64 torch restatement below, written from the definitions in include/vargp_hip.h:
    softmax    p_sf = softmax_c(mu_s + sqrt(var_s) eps_sf);  probs = mean_sf p_sf;  total = -sum_c probs log probs (0 log 0 = 0);
               expected = mean_sf( -sum_c p_sf log p_sf ) from log-probabilities;  mi = max(total - expected, 0)
    bernoulli  per output, 20-node rule (w^_k, f_k = mu + sqrt(2 var) x_k), either link:  p_out = mean_s sum_k w^_k Lambda(f_k),
               1 - p_out = mean_s sum_k w^_k Lambda(-f_k),  total_out = h(p_out),  expected_out = mean_s sum_k w^_k h(Lambda(f_k))
               from log Lambda(+-f_k),  mi_out = max(total_out - expected_out, 0);  total, expected, mi = their sums over c

Op-level bound: rel_l2 <= 1e-5 against fp64 for every output (mi included) on every case, the project's op-level bound for
kernels that compute in fp64 and round once (tests/test_hip_lpd.py).  Where the definition makes a vector identically zero
(_is_zero: the softmax's mi at S F = 1 or C = 1 and its entropies at C = 1; the Bernoulli mi at S = 1 and var = 0, where the
rule has one node value) the fp64 restatement gives 0 up to its own rounding (<= 1e-15) and max |out| <= 1e-6 is required instead.
The CPU table (test_fp32_restatement_keeps_its_digits) evaluates the same restatement in plain fp32 on every GPU case.  Measured
here, worst rel_l2 against fp64 over all cases: 1.3e-7 for probs, total and expected, and 9.7e-7 for mi and mi_out (a difference
of two fp32 entropies, so a few times their error).  The hyper-samples of the table disagree with each other, so mi is a sizeable part
of total on every case, mu8 included (there the samples are confident of DIFFERENT classes: mi is most of total); no case
needs the absolute floor beyond the identically-zero ones, none needs slack and none is left out."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import rel_l2

gpu = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(1, 1, 1), (3, 3, 63), (2, 5, 65), (5, 17, 130), (64, 2, 70)]     # one lane | partial wave | wave + 1 | C > 16, three
KINDS = ['typical', 'var0', 'var25', 'mu8']                                 # point blocks | more (hyper-)samples than waves
SOFTMAX_F = [1, 4]
LINKS = ['probit', 'logit']
BOUND = 1e-5
FLOOR = 1e-6
SM_NAMES = ('probs', 'total', 'expected', 'mi')
BE_NAMES = SM_NAMES + ('total_out', 'expected_out', 'mi_out')
ids_shape = lambda s: 'S%d-C%d-B%d' % s


# -- the restatement (any dtype; fp64 is the yardstick) -------------------------------------------------------------------------
def _entropy(p):
    return -torch.xlogy(p, p)                                    # 0 log 0 = 0


def softmax_unc(mu, var, eps):
    """mu, var (S, C, B), eps (S, F, C, B) -> probs (B, C), total, expected, mi (B,)."""
    logp = torch.log_softmax(mu.unsqueeze(1) + var.sqrt().unsqueeze(1) * eps, dim=2)     # f - Z: finite, log(0) never taken
    p = logp.exp()
    probs = p.mean((0, 1))
    total = _entropy(probs).sum(0)
    expected = (-(p * logp).sum(2)).mean((0, 1))
    return probs.t(), total, expected, (total - expected).clamp_min(0)


def bernoulli_unc(mu, var, link):
    """mu, var (S, C, B) -> probs (B, C), total, expected, mi (B,), total_out, expected_out, mi_out (C, B)."""
    x, w = np.polynomial.hermite.hermgauss(20)
    x, w = torch.tensor(x, dtype=mu.dtype), torch.tensor(w / np.sqrt(np.pi), dtype=mu.dtype)
    f = mu.unsqueeze(-1) + (2 * var).sqrt().unsqueeze(-1) * x
    log_link = torch.special.log_ndtr if link == 'probit' else torch.nn.functional.logsigmoid
    lp, lm = log_link(f), log_link(-f)
    ep, em = lp.exp(), lm.exp()
    p, q = (w * ep).sum(-1).mean(0), (w * em).sum(-1).mean(0)
    e = (-(w * (ep * lp + em * lm)).sum(-1)).mean(0)
    t = _entropy(p) + _entropy(q)
    m = (t - e).clamp_min(0)
    return p.t(), t.sum(0), e.sum(0), m.sum(0), t, e, m


# -- inputs: the table of the op-level tests ------------------------------------------------------------------------------------
def inputs(shape, kind, F=None):
    """-> mu, var (S, C, B) fp32 and, with F, eps (S, F, C, B): the moments of tests/test_hip_lpd.py's table."""
    S, C, B = shape
    gen = torch.Generator().manual_seed(1 + 1000 * S + 10 * C + B)
    mu = torch.randn(S, C, B, generator=gen)
    var = 0.01 + 0.5 * torch.rand(S, C, B, generator=gen)
    if kind == 'var0':
        var = torch.zeros_like(var)
    elif kind == 'var25':
        var = torch.full_like(var, 25.0)
    elif kind == 'mu8':
        mu = 8 * mu
    if F is None:
        return mu, var
    return mu, var, torch.randn(S, F, C, B, generator=gen)


@functools.lru_cache(maxsize=None)
def reference(lik, shape, kind, dtype=torch.float64):
    """The restatement of one case on the CPU: computed once, shared by every test that needs it.  lik: 'probit' | 'logit' |
    the softmax's F."""
    if lik in LINKS:
        return bernoulli_unc(*(a.to(dtype) for a in inputs(shape, kind)), lik)
    return softmax_unc(*(a.to(dtype) for a in inputs(shape, kind, lik)))


CASES = [(lik, shape, kind) for lik in SOFTMAX_F + LINKS for shape in SHAPES for kind in KINDS]


# -- CPU --------------------------------------------------------------------------------------------------------------------------
def test_restatement_hand_values():
    d = torch.float64
    gen = torch.Generator().manual_seed(5)
    # one sample: nothing to disagree with
    mu, var = torch.randn(1, 4, 9, generator=gen, dtype=d), torch.rand(1, 4, 9, generator=gen, dtype=d)
    _, total, expected, mi = softmax_unc(mu, var, torch.randn(1, 1, 4, 9, generator=gen, dtype=d))
    assert torch.equal(mi, torch.zeros_like(mi)) and rel_l2(total, expected) < 1e-14 and (total > 0).all()
    # one class: nothing to be unsure about
    out = softmax_unc(mu[:, :1], var[:, :1], torch.randn(1, 3, 1, 9, generator=gen, dtype=d))
    assert torch.equal(out[0], torch.ones(9, 1, dtype=d)) and all(torch.equal(o, torch.zeros(9, dtype=d)) for o in out[1:])
    # uniform logits without variance: log C, all of it noise
    C = 7
    _, total, expected, mi = softmax_unc(torch.full((2, C, 3), 0.3, dtype=d), torch.zeros(2, C, 3, dtype=d),
                                         torch.randn(2, 2, C, 3, generator=gen, dtype=d))
    assert (total - math.log(C)).abs().max() < 1e-14 and (expected - math.log(C)).abs().max() < 1e-14 and mi.max() < 1e-14
    # a Bernoulli output at mu = 0, var = 0: log 2, all of it noise
    for link in LINKS:
        out = bernoulli_unc(torch.zeros(1, 1, 1, dtype=d), torch.zeros(1, 1, 1, dtype=d), link)
        assert abs(out[4].item() - math.log(2)) < 1e-14 and abs(out[5].item() - math.log(2)) < 1e-14 and out[6].item() < 1e-14
        assert abs(out[0].item() - 0.5) < 1e-15
    # two hyper-samples, each certain of another class: log 2, all of it lack of knowledge
    mu = torch.tensor([[[40.0], [-40.0]], [[-40.0], [40.0]]], dtype=d)              # (S = 2, C = 2, B = 1)
    probs, total, expected, mi = softmax_unc(mu, torch.zeros_like(mu), torch.zeros(2, 1, 2, 1, dtype=d))
    assert abs(total.item() - math.log(2)) < 1e-14 and abs(mi.item() - math.log(2)) < 1e-14 and abs(expected.item()) < 1e-14
    assert (probs - 0.5).abs().max() < 1e-15
    # |f| = 30: finite and tiny, from the log-probabilities
    for link in LINKS:
        out = bernoulli_unc(torch.tensor([[[30.0, -30.0]]], dtype=d), torch.zeros(1, 1, 2, dtype=d), link)
        assert all(torch.isfinite(o).all() for o in out) and 0 < out[5].max() < 1e-10


def test_restatement_jensen_holds_on_every_case():
    for lik, shape, kind in CASES:
        ref = reference(lik, shape, kind)
        assert all(torch.isfinite(o).all() for o in ref), (lik, shape, kind)
        assert (ref[1] - ref[2]).min() >= -1e-12, (lik, shape, kind)
        if lik in LINKS:
            assert (ref[4] - ref[5]).min() >= -1e-12, (lik, shape, kind)
        else:
            assert ref[1].max() <= math.log(shape[1]) + 1e-12 and ref[2].min() >= -1e-12


def _is_zero(lik, shape, kind, name):
    """Is this output identically zero by definition (module docstring)?"""
    S, C, _ = shape
    if lik in LINKS:
        return name.startswith('mi') and S == 1 and kind == 'var0'
    return C == 1 and name != 'probs' or name == 'mi' and S * lik == 1


@pytest.mark.parametrize('shape', SHAPES, ids=ids_shape)
def test_fp32_restatement_keeps_its_digits(shape):
    """Every case of the op-level table: plain fp32 arithmetic stays within 1e-4 of fp64 (measured: 1e-6, module docstring), so
    the 1e-5 bound on a kernel that rounds once needs no per-kind slack."""
    worst, worst_mi = 0.0, 0.0
    for kind in KINDS:
        for lik in SOFTMAX_F + LINKS:
            r64, r32 = reference(lik, shape, kind), reference(lik, shape, kind, torch.float32)
            for name, a, b in zip(BE_NAMES, r32, r64):
                assert torch.isfinite(a).all(), (lik, kind, name)
                if _is_zero(lik, shape, kind, name):
                    assert b.abs().max() <= 1e-15 and a.abs().max() <= FLOOR, (lik, kind, name)
                    continue
                e = rel_l2(a, b)
                assert e < 1e-4, (lik, kind, name, e)
                if name.startswith('mi'):
                    worst_mi = max(worst_mi, e)
                else:
                    worst = max(worst, e)
    print(f'[fp32 restatement] {ids_shape(shape)}: worst rel_l2 {worst:.2e}, of mi {worst_mi:.2e}', flush=True)


def test_ops_check_their_arguments_before_the_device():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    from vargp_amd.likelihoods import (BernoulliLikelihood, GaussianLikelihood, MulticlassSoftmax, PoissonLikelihood,
                                       StudentTLikelihood)
    mu, var, eps = torch.zeros(2, 3, 4), torch.ones(2, 3, 4), torch.zeros(2, 5, 3, 4)
    for call in (lambda: ops.softmax_uncertainty(mu, var, eps[:, :, :2]),                     # eps of another C
                 lambda: ops.softmax_uncertainty(mu, var, eps[0]),                           # eps without its sample dims
                 lambda: ops.softmax_uncertainty(mu, var[:1], eps),
                 lambda: ops.softmax_uncertainty(mu.double(), var.double(), eps.double()),
                 lambda: ops.softmax_uncertainty(mu, var, eps.double()),
                 lambda: ops.bernoulli_uncertainty(mu[0], var[0]),
                 lambda: ops.bernoulli_uncertainty(mu, var[..., :3]),
                 lambda: ops.bernoulli_uncertainty(mu.double(), var.double()),
                 lambda: ops.bernoulli_uncertainty(mu[:, :0], var[:, :0])):
        with pytest.raises(AssertionError):
            call()
    with pytest.raises(ValueError, match='link'):
        ops.bernoulli_uncertainty(mu, var, 'cloglog')
    for call in (lambda: ops.softmax_uncertainty(mu, var, eps), lambda: ops.bernoulli_uncertainty(mu, var, 'logit')):
        with pytest.raises(VargpHipError):                                                   # well-formed, but no CPU path
            call()
    with pytest.raises(ValueError, match='per-output'):
        MulticlassSoftmax(n_f=2).uncertainty(mu, var, per_output=True)
    for lik in (GaussianLikelihood(3), StudentTLikelihood(3), PoissonLikelihood()):
        with pytest.raises(ValueError, match=type(lik).__name__):
            lik.uncertainty(mu, var)
    assert BernoulliLikelihood.uncertainty is not GaussianLikelihood.uncertainty


def test_c_abi_argument_checks_need_no_device():
    """Every argument error returns before any launch (nothing here touches a device), with vargp_last_error naming the entry."""
    from vargp_amd._lib import lib
    L, p = lib(), 64                                        # (p: a non-NULL, 8-byte aligned pointer value, never dereferenced)
    need = L.vargp_softmax_uncertainty_workspace_bytes(2, 3, 17, 5)
    assert need == (2 * 3 + 1) * 5 * 8                      # S F B + B doubles: no factor C
    sm = lambda *a: L.vargp_softmax_uncertainty(*a, None)
    bad = [(None, p, p, p, p, p, p, 2, 3, 17, 5, p, need), (p, None, p, p, p, p, p, 2, 3, 17, 5, p, need),
           (p, p, None, p, p, p, p, 2, 3, 17, 5, p, need), (p, p, p, p, None, p, p, 2, 3, 17, 5, p, need),
           (p, p, p, p, p, None, p, 2, 3, 17, 5, p, need), (p, p, p, p, p, p, None, 2, 3, 17, 5, p, need),
           (p, p, p, p, p, p, p, 0, 3, 17, 5, p, need), (p, p, p, p, p, p, p, 2, 0, 17, 5, p, need),
           (p, p, p, p, p, p, p, 2, 3, 0, 5, p, need), (p, p, p, p, p, p, p, 2, 3, 17, -1, p, need),
           (p, p, p, p, p, p, p, 2, 3, 17, 5, None, need), (p, p, p, p, p, p, p, 2, 3, 17, 5, p, need - 1),
           (p, p, p, p, p, p, p, 2, 3, 17, 5, p + 4, need)]
    for args in bad:
        L.vargp_bernoulli_uncertainty(None, None, 0, None, None, None, None, None, None, None, 1, 1, 1, None)   # another message
        assert sm(*args) != 0, args
        assert b'softmax_uncertainty' in L.vargp_last_error(), args
    be = lambda *a: L.vargp_bernoulli_uncertainty(*a, None)
    bad = [(None, p, 0, p, p, p, p, p, p, p, 1, 1, 1), (p, None, 0, p, p, p, p, p, p, p, 1, 1, 1),
           (p, p, 0, p, None, p, p, p, p, p, 1, 1, 1), (p, p, 0, p, p, None, p, p, p, p, 1, 1, 1),
           (p, p, 0, p, p, p, None, p, p, p, 1, 1, 1), (p, p, 2, p, p, p, p, p, p, p, 1, 1, 1),
           (p, p, -1, p, p, p, p, p, p, p, 1, 1, 1), (p, p, 1, p, p, p, p, p, p, p, 0, 1, 1),
           (p, p, 1, p, p, p, p, p, p, p, 1, 0, 1), (p, p, 1, p, p, p, p, p, p, p, 1, 1, 0)]
    for args in bad:
        sm(None, p, p, p, p, p, p, 1, 1, 1, 1, p, 64)
        assert be(*args) != 0, args
        assert b'bernoulli_uncertainty' in L.vargp_last_error(), args


# -- GPU, op level ----------------------------------------------------------------------------------------------------------------
def _check(what, got, case, names):
    errs, ref = [], reference(*case)
    for name, a, b in zip(names, got, ref):
        assert a.shape == b.shape and torch.isfinite(a).all(), (what, name, a.shape, b.shape)
        if _is_zero(*case, name):
            e = a.abs().max().item()
            assert e <= FLOOR, (what, name, e)
            errs.append(f'{name} |{e:.1e}|')
        else:
            e = rel_l2(a, b)
            errs.append(f'{name} {e:.1e}')
            assert e <= BOUND, (what, name, e)
    print(f'[op] {what}: ' + ' '.join(errs), flush=True)


def _invariants(what, out, C, softmax):
    probs, total, expected, mi = out[:4]
    assert (mi >= 0).all() and (expected <= total + 1e-6).all(), what
    if softmax:
        assert (probs.double().sum(1) - 1).abs().max() <= 1e-6, what
        assert (total <= math.log(C) + 1e-6).all(), what
    elif len(out) > 4:
        for joint, per in zip(out[1:4], out[4:]):
            assert (per >= 0).all() and per.shape == (C, joint.shape[0]), what
            assert rel_l2(per.double().sum(0), joint) <= 1e-6, (what, rel_l2(per.double().sum(0), joint))


def _raw_softmax_no_probs(mu, var, eps):
    from vargp_amd._lib import check, lib, ptr, scratch, stream_ptr
    S, F, C, B = eps.shape
    out = [torch.empty(B, device=DEV) for _ in range(3)]
    ws = scratch(lib().vargp_softmax_uncertainty_workspace_bytes(S, F, C, B), mu.device)
    check(lib().vargp_softmax_uncertainty(ptr(mu), ptr(var), ptr(eps), None, *(ptr(o) for o in out), S, F, C, B, ptr(ws),
                                          ws.numel() * 4, stream_ptr()), 'vargp_softmax_uncertainty')
    return out


def _raw_bernoulli_no_probs(mu, var, link, per_output):
    from vargp_amd._lib import check, lib, ptr, stream_ptr
    S, C, B = mu.shape
    out = [torch.empty(B, device=DEV) for _ in range(3)] + ([torch.empty(C, B, device=DEV) for _ in range(3)] if per_output else [])
    args = [ptr(o) for o in out] + [None] * (6 - len(out))
    check(lib().vargp_bernoulli_uncertainty(ptr(mu), ptr(var), link, None, *args, S, C, B, stream_ptr()),
          'vargp_bernoulli_uncertainty')
    return out


@gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=ids_shape)
def test_softmax_op_vs_fp64(shape, kind):
    from vargp_amd import ops
    S, C, B = shape
    for F in SOFTMAX_F:
        what = f'softmax F{F} {ids_shape(shape)} {kind}'
        mu, var, eps = (a.to(DEV) for a in inputs(shape, kind, F))
        a, b = ops.softmax_uncertainty(mu, var, eps), ops.softmax_uncertainty(mu, var, eps)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), what                    # no float atomics: bitwise reproducible
        _check(what, [o.cpu() for o in a], (F, shape, kind), SM_NAMES)
        _invariants(what, a, C, softmax=True)
        assert (a[0] - ops.softmax_predict(mu, var, eps)).abs().max().item() <= 1e-6, what
        for p, q in zip(_raw_softmax_no_probs(mu, var, eps), a[1:]):                 # probs = NULL changes nothing else
            assert torch.equal(p, q), what


@gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=ids_shape)
def test_bernoulli_op_vs_fp64(shape, kind):
    from vargp_amd import ops
    S, C, B = shape
    mu, var = (a.to(DEV) for a in inputs(shape, kind))
    for link in LINKS:
        what = f'{link} {ids_shape(shape)} {kind}'
        a, b = ops.bernoulli_uncertainty(mu, var, link, per_output=True), ops.bernoulli_uncertainty(mu, var, link, per_output=True)
        assert len(a) == 7 and all(torch.equal(p, q) for p, q in zip(a, b)), what
        _check(what, [o.cpu() for o in a], (link, shape, kind), BE_NAMES)
        _invariants(what, a, C, softmax=False)
        short = ops.bernoulli_uncertainty(mu, var, link)
        assert len(short) == 4 and all(torch.equal(p, q) for p, q in zip(short, a)), what
        for per_output in (False, True):                                             # probs = NULL changes nothing else
            raw = _raw_bernoulli_no_probs(mu, var, ops.BERNOULLI_LINKS[link], per_output)
            assert all(torch.equal(p, q) for p, q in zip(raw, a[1:])), what


@gpu
def test_undersized_workspace_is_refused_before_any_launch():
    from vargp_amd._lib import lib, ptr, stream_ptr
    S, F, C, B = 2, 3, 4, 70
    mu, var, eps = (a.to(DEV) for a in inputs((S, C, B), 'typical', F))
    out = [torch.full((B,), -7.0, device=DEV) for _ in range(3)]
    need = lib().vargp_softmax_uncertainty_workspace_bytes(S, F, C, B)
    ws = torch.empty(need // 4, device=DEV)
    rc = lib().vargp_softmax_uncertainty(ptr(mu), ptr(var), ptr(eps), None, *(ptr(o) for o in out), S, F, C, B, ptr(ws), need - 8,
                                         stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and b'softmax_uncertainty' in lib().vargp_last_error()
    assert all((o == -7.0).all() for o in out)                                       # nothing ran


# -- GPU, model level -----------------------------------------------------------------------------------------------------------
def _model(lik, n_prev, N, F=4, seed=61):
    import test_hip_lpd
    assert test_hip_lpd.SOFTMAX_F == F
    _build = test_hip_lpd._build
    S, C, M, D = 2, 3, 12, 8
    params, prev, x, labels, nz = orc.make_problem(S, F, C, M, D, N, n_prev=n_prev, seed=seed + n_prev, kind='gauss')
    return _build(params, prev, S, lik), x.to(DEV), nz


@gpu
@pytest.mark.parametrize('lik,n_prev', [('softmax', 0), ('softmax', 1), ('probit', 1), ('logit', 0)])
def test_model_uncertainty(lik, n_prev):
    """VARGP.uncertainty = the restatement on the model's own predict_f moments, to the bound of tests/test_hip_lpd.py's
    model-level comparison (1e-5)."""
    from vargp_amd import noise
    from vargp_amd.likelihoods import Uncertainty
    N, C = 70, 3
    gp, x, nz = _model(lik, n_prev, N)
    inj = dict(eps_theta=nz['eps_theta'].to(DEV))
    if lik == 'softmax':
        inj['eps_f'] = nz['eps_f'].to(DEV)
    with noise.inject(**inj):
        u = gp.uncertainty(x)
        mu, var = gp.predict_f(x)
        pred = gp.predict(x)
    assert isinstance(u, Uncertainty) and u.total_out is None and not any(t.requires_grad for t in u[:4])
    assert u.probs.shape == (N, C) and u.total.shape == u.aleatoric.shape == u.epistemic.shape == (N,)
    if lik == 'softmax':
        want = softmax_unc(mu.cpu().double(), var.cpu().double(), nz['eps_f'].double())
        assert (u.probs - pred).abs().max().item() <= 1e-6
        with pytest.raises(ValueError):
            gp.uncertainty(x, per_output=True)
    else:
        want = bernoulli_unc(mu.cpu().double(), var.cpu().double(), lik)
        with noise.inject(**inj):
            u = gp.uncertainty(x, per_output=True)
        assert u.total_out.shape == u.aleatoric_out.shape == u.epistemic_out.shape == (C, N)
    errs = [rel_l2(a.cpu(), b) for a, b in zip(u, want)]
    print(f'[model] {lik} n_prev {n_prev}: ' + ' '.join(f'{e:.1e}' for e in errs), flush=True)
    assert all(e <= 1e-5 for e in errs), errs
    _invariants(f'model {lik}', tuple(u) if lik != 'softmax' else tuple(u[:4]), C, softmax=lik == 'softmax')


@gpu
@pytest.mark.parametrize('n_prev', [0, 1])
def test_tiled_bernoulli_uncertainty_equals_the_single_call(n_prev):
    from vargp_amd import noise
    N, C = 70, 3
    gp, x, nz = _model('probit', n_prev, N)
    with noise.inject(eps_theta=nz['eps_theta'].to(DEV)):
        one, tiled = gp.uncertainty(x, per_output=True), gp.uncertainty(x, tile=32, per_output=True)
        short = gp.uncertainty(x, tile=32)
    assert short.total_out is None and all(torch.equal(a, b) for a, b in zip(short[:4], tiled[:4]))
    for name, a, b in zip(one._fields, tiled, one):
        assert a.shape == b.shape, name
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=1e-6, atol=1e-6, err_msg=name)


@gpu
def test_tiled_softmax_uncertainty_shapes_and_invariants():
    N, C = 70, 3
    gp, x, _ = _model('softmax', 1, N)
    torch.manual_seed(0)
    u = gp.uncertainty(x, tile=32)                                                   # (the tiles draw their own eps_f)
    assert u.probs.shape == (N, C) and all(t.shape == (N,) for t in u[1:4]) and u.total_out is None
    _invariants('tiled softmax', tuple(u[:4]), C, softmax=True)


@gpu
def test_compute_uncertainty_is_the_mean_over_the_points():
    from test_hip_reg_lik import _Data
    from vargp_amd import noise
    from vargp_amd.train_utils import compute_uncertainty
    N = 70
    gp, x, nz = _model('logit', 1, N)
    data = _Data(x.cpu(), torch.zeros(N, dtype=torch.int64))
    with noise.inject(eps_theta=nz['eps_theta'].to(DEV)):
        u = gp.uncertainty(x)
        got = compute_uncertainty(data, gp, batch_size=32, device=DEV)               # three batches: 32, 32, 6
        shared = compute_uncertainty(data, gp, batch_size=32, device=DEV, shared_hypers=True)
    want = [t.double().mean().item() for t in (u.total, u.aleatoric, u.epistemic)]
    np.testing.assert_allclose(got, want, rtol=1e-5)
    np.testing.assert_allclose(shared, want, rtol=1e-5)
    assert want[0] >= want[2] >= 0


@gpu
def test_driver_logs_entropy_and_mutual_information(tmp_path):
    from test_hip_driver import _run
    log, sc = _run(['s-mnist', '--synthetic', '--n_synth', '3000', '--epochs', '2', '--eval_interval', '2', '--M', '20',
                    '--uncertainty', '--seed', '2'], tmp_path)
    for t in range(5):
        ent, mi = sc[(f'task{t}/test/entropy', 2)], sc[(f'task{t}/test/mi', 2)]
        assert math.isfinite(ent) and math.isfinite(mi) and ent >= mi >= 0, (t, ent, mi)
    assert not any('lpd' in k for k, _ in sc)
