"""GPU: the per-op kernels of the composed route at their branch and shape edges, each against an fp64 host reference (the
oracle's function where it has one, else torch fp64 autograd on the reference's formula), on seeded inputs.  What
tests/test_hip_ops.py checks at one shape, this file checks where kernels go wrong: both backward kernels of the softmax
likelihood (C <= 16 and the generic one), one gradient at a time into the Cholesky backward, the strided `a` of the predictive
moments (a C-ABI form `ops` never passes), reductions past one 256-thread block, the softplus threshold, ragged 64-wide tiles
and exact zeros of ReLU.  Tolerances are fp32-level and written per test."""
import numpy as np
import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import rel_l2

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _hn(shape, seed, scale=1.0):
    return (scale * orc.hash_normal(shape, seed)).float()


def _hu(shape, seed, lo=0.0, hi=1.0):
    return (lo + (hi - lo) * orc.hash_uniform(shape, seed)).float()


def _d64(t):
    return t.detach().cpu().double().requires_grad_(True)


@pytest.fixture(scope='module')
def ops():
    from vargp_amd import ops as o
    return o


# ---- Monte-Carlo softmax likelihood ---------------------------------------------------------------------------
@pytest.mark.parametrize('F', [1, 3, 17])
@pytest.mark.parametrize('C', [1, 2, 15, 16, 17, 33])
def test_softmax_likelihood_edges(ops, C, F):
    """C <= 16: the register-resident backward with atomics; C > 16: the generic per-(s, c, b) backward.  S F B and S C B are
    no multiples of 256 (3 x 67 = 201 columns per class or sample), logits spread over +-80 (exp without the max subtracted
    overflows), var down to 1e-6, labels on every class, the first and the last included."""
    S, B = 3, 67
    mu = _hu((S, C, B), 10 * C + F, -80.0, 80.0)
    var = (10.0 ** _hu((S, C, B), 11 * C + F, -6.0, 0.0)).float()
    eps = _hn((S, F, C, B), 12 * C + F)
    y = torch.arange(B) % C
    y[0], y[-1] = C - 1, 0
    mu_d, var_d = mu.to(DEV).requires_grad_(True), var.to(DEV).requires_grad_(True)
    nll = ops.softmax_nll(mu_d, var_d, eps.to(DEV), y.to(DEV))
    (3.0 * nll).backward()
    mu64, var64 = _d64(mu), _d64(var)
    ref = orc.softmax_nll(mu64, var64, y, eps.double())
    (3.0 * ref).backward()
    # per term |f| <= ~80 + 4: fp32 rounding of f and of the log-sum-exp ~1e-5 absolute
    assert abs(nll.item() - ref.item()) <= 1e-6 * abs(ref.item()) + 2e-5 * B, (nll.item(), ref.item())
    assert torch.isfinite(mu_d.grad).all() and torch.isfinite(var_d.grad).all()
    assert rel_l2(mu_d.grad.cpu(), mu64.grad) < 5e-5
    assert rel_l2(var_d.grad.cpu(), var64.grad) < 5e-5

    probs = ops.softmax_predict(mu_d.detach(), var_d.detach(), eps.to(DEV))
    pref = orc.softmax_predict(mu64.detach(), var64.detach(), eps.double())
    assert probs.shape == (B, C)
    np.testing.assert_allclose(probs.cpu().numpy(), pref.numpy(), rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(probs.double().sum(-1).cpu().numpy(), np.ones(B), rtol=0, atol=2e-5)


# ---- Cholesky backward with one of its two gradients ----------------------------------------------------------
def _spd(nb, n, seed):
    A = orc.hash_normal((nb, n, n + 8), seed)
    return ((A @ A.mT) / (n + 8) + 0.05 * torch.eye(n, dtype=torch.float64)).float()


def _ref_LT(A, eps):
    n = A.shape[-1]
    A64 = A.double().requires_grad_(True)
    L64 = torch.linalg.cholesky(A64 + eps * torch.eye(n, dtype=torch.float64))
    T64 = torch.linalg.solve_triangular(L64, torch.eye(n, dtype=torch.float64).expand_as(L64), upper=False)
    return A64, L64, T64


CHOL_NS = [1, 20, 64, 65, 100, 101, 150, 257]


@pytest.mark.parametrize('n', CHOL_NS)
def test_chol_backward_without_inverse_gradient(ops, n):
    """ops.chol (want_inv=False): the backward gets gT = NULL -- what gp_utils.cholesky and the composed routes take.  The
    weights are full matrices: the part above the diagonal must not reach gA."""
    nb = 3
    A = _spd(nb, n, 400 + n)
    A_d = A.to(DEV).requires_grad_(True)
    L = ops.chol(A_d, 1e-4)
    wl = _hn(L.shape, 401 + n)
    (L * wl.to(DEV)).sum().backward()
    A64, L64, _ = _ref_LT(A, 1e-4)
    (L64 * wl.double()).sum().backward()
    assert rel_l2(L.detach().cpu(), L64.detach()) < 1e-5
    assert rel_l2(A_d.grad.cpu(), A64.grad) < 1e-3


@pytest.mark.parametrize('n', CHOL_NS)
def test_chol_inv_bwd_c_abi_one_gradient(ops, n):
    """vargp_chol_inv_bwd with gL = NULL (a caller that uses only T), and with both gradients, on the same factor."""
    from vargp_amd._lib import check, lib, ptr, scratch, stream_ptr
    nb = 3
    A = _spd(nb, n, 500 + n)
    with torch.no_grad():
        L, T = ops.chol_inv(A.to(DEV), 1e-4)
    wl, wt = _hn(L.shape, 501 + n), _hn(L.shape, 502 + n)
    ws = scratch(lib().vargp_chol_workspace_bytes(nb, n, 1), L.device)

    def bwd(gL, gT):
        gA = torch.full_like(L, float('nan'))
        check(lib().vargp_chol_inv_bwd(ptr(L), ptr(T), ptr(gL), ptr(gT), ptr(gA), nb, n, ptr(ws), ws.numel() * 4,
                                       stream_ptr()), 'vargp_chol_inv_bwd')
        return gA.cpu()

    gA_t = bwd(None, wt.to(DEV))
    gA_lt = bwd(wl.to(DEV), wt.to(DEV))
    A64, L64, T64 = _ref_LT(A, 1e-4)
    ref_t, = torch.autograd.grad((T64 * wt.double().tril()).sum(), A64, retain_graph=True)
    ref_lt, = torch.autograd.grad((T64 * wt.double().tril()).sum() + (L64 * wl.double()).sum(), A64)
    assert rel_l2(gA_t, ref_t) < 1e-3
    assert rel_l2(gA_lt, ref_lt) < 1e-3


# ---- predictive moments with a strided `a` (C ABI) ------------------------------------------------------------
@pytest.mark.parametrize('M', [1, 3, 100])
@pytest.mark.parametrize('B', [1, 63, 64, 65, 513])
@pytest.mark.parametrize('layout', ['column', 'wide_batch'])
def test_predictive_diag_strided_a(ops, B, M, layout):
    """`a` read as column 2 of a wider (nb, M, 5) matrix (a_stride = 5, a_bstride = 5 M), or as rows of an (nb, M + 7) matrix
    (a_stride = 1, a_bstride = M + 7) -- include/vargp_hip.h documents both; ops.predictive_diag always passes (1, M)."""
    from vargp_amd._lib import check, lib, ptr, stream_ptr
    nb = 6
    P, W = _hn((nb, M, B), 600 + B + M), _hn((nb, M, B), 601 + B + M)
    kd = (1.0 + orc.hash_uniform((nb,), 602)).float()
    if layout == 'column':
        a_store = _hn((nb, M, 5), 603 + M)
        a, a_stride, a_bstride = a_store[..., 2], 5, 5 * M
    else:
        a_store = _hn((nb, M + 7), 603 + M)
        a, a_stride, a_bstride = a_store[..., :M], 1, M + 7
    gmu, gvar = _hn((nb, B), 604), _hn((nb, B), 605)
    Pd, Wd, kdd, gmud, gvard = (t.to(DEV).contiguous() for t in (P, W, kd, gmu, gvar))
    a_dev = a_store.to(DEV)
    a_view = a_dev[..., 2] if layout == 'column' else a_dev[..., :M]
    mu, var = (torch.full((nb, B), float('nan'), device=DEV) for _ in range(2))
    check(lib().vargp_predictive_diag_fwd(ptr(Pd), ptr(Wd), ptr(a_view), a_stride, a_bstride, ptr(kdd), ptr(mu), ptr(var),
                                          nb, M, B, stream_ptr()), 'vargp_predictive_diag_fwd')
    gP, gW = torch.full_like(Pd, float('nan')), torch.full_like(Wd, float('nan'))
    ga, gk = torch.full((nb, M), float('nan'), device=DEV), torch.full((nb,), float('nan'), device=DEV)
    check(lib().vargp_predictive_diag_bwd(ptr(Pd), ptr(Wd), ptr(a_view), a_stride, a_bstride, ptr(gmud), ptr(gvard), ptr(gP),
                                          ptr(gW), ptr(ga), ptr(gk), nb, M, B, stream_ptr()), 'vargp_predictive_diag_bwd')
    torch.cuda.synchronize()
    assert torch.equal(a_dev.cpu(), a_store)                     # the wider matrix is read only

    t64 = [t.double().requires_grad_(True) for t in (P, W, a.contiguous(), kd)]
    mu64 = (t64[0] * t64[2].unsqueeze(-1)).sum(-2)
    var64 = t64[3].unsqueeze(-1) - t64[0].pow(2).sum(-2) + t64[1].pow(2).sum(-2)
    ((mu64 * gmu.double()).sum() + (var64 * gvar.double()).sum()).backward()
    assert rel_l2(mu.cpu(), mu64.detach()) < 2e-6 and rel_l2(var.cpu(), var64.detach()) < 2e-6
    for got, ref in zip((gP, gW, ga, gk), t64):
        assert rel_l2(got.cpu(), ref.grad) < 2e-6


# ---- MVN KL from its factors, log-determinant of a triangle ---------------------------------------------------
def _tril_spread(nb, n, seed):
    """Lower triangles with diagonals log-spread over 1e-3..1e3 and rows scaled by their diagonal (L = D (I + E))."""
    dg = 10.0 ** (-3.0 + 6.0 * orc.hash_uniform((nb, n), seed))
    E = (0.3 / n ** 0.5) * orc.hash_normal((nb, n, n), seed + 1).tril(-1)
    return dg.unsqueeze(-1) * (torch.eye(n, dtype=torch.float64) + E)


KL_MS = [1, 17, 63, 64, 65, 100, 300]


@pytest.mark.parametrize('M', KL_MS)
def test_mvn_kl_and_logdet_edges(ops, M):
    """ops.mvn_kl_from_factors + ops.logdet_tril (the KL of gp_utils.mvn_kl) against orc.mvn_kl in fp64, up to 30 batches.
    d = Lp^-1 (mu_q - mu_p) is drawn so that every entry of d weighs as much as a row of G in the trace term: a reduction that
    dropped part of d (M > 256: more than one pass of the block) shows."""
    nb = 30 if M <= 100 else 8
    Lp, Lq = _tril_spread(nb, M, 700 + M), _tril_spread(nb, M, 720 + M)
    G64 = torch.linalg.solve_triangular(Lp, Lq, upper=False)
    zd = orc.hash_normal((nb, M), 740 + M) * (G64.pow(2).sum((-2, -1)) / M).sqrt().unsqueeze(-1)
    mu_p = orc.hash_normal((nb, M), 741 + M)
    mu_q = mu_p + (Lp @ zd.unsqueeze(-1)).squeeze(-1)
    d64 = torch.linalg.solve_triangular(Lp, (mu_q - mu_p).unsqueeze(-1), upper=False).squeeze(-1)
    ref = orc.mvn_kl(mu_q, Lq, mu_p, Lp)

    G, d = G64.float().to(DEV).requires_grad_(True), d64.float().to(DEV).requires_grad_(True)
    Lp_d, Lq_d = Lp.float().to(DEV).requires_grad_(True), Lq.float().to(DEV).requires_grad_(True)
    ldp, ldq = ops.logdet_tril(Lp_d), ops.logdet_tril(Lq_d)
    kl = ops.mvn_kl_from_factors(G, d, ldp, ldq)
    assert kl.shape == (nb,)
    # scale of the terms the kernel adds: |log det| and the trace / Mahalanobis sums
    logs = Lp.diagonal(dim1=-2, dim2=-1).log().abs().sum(-1) + Lq.diagonal(dim1=-2, dim2=-1).log().abs().sum(-1)
    scale = logs + 0.5 * (G64.pow(2).sum((-2, -1)) + d64.pow(2).sum(-1) + M)
    assert ((kl.detach().cpu().double() - ref).abs() <= 2e-6 * scale).all(), (kl.detach().cpu().double() - ref) / scale
    ld_ref = Lp.diagonal(dim1=-2, dim2=-1).log().sum(-1)
    assert ((ldp.detach().cpu().double() - ld_ref).abs() <= 1e-6 * Lp.diagonal(dim1=-2, dim2=-1).log().abs().sum(-1) + 1e-6).all()

    w = _hn((nb,), 742 + M)
    (kl * w.to(DEV)).sum().backward()
    t64 = [t.double().requires_grad_(True) for t in (G64.float(), d64.float(), Lp.float(), Lq.float())]
    ld64 = [t.diagonal(dim1=-2, dim2=-1).log().sum(-1) for t in t64[2:]]
    kl64 = ld64[0] - ld64[1] + 0.5 * (t64[0].pow(2).sum((-2, -1)) + t64[1].pow(2).sum(-1) - M)
    (kl64 * w.double()).sum().backward()
    for got, r in zip((G, d, Lp_d, Lq_d), t64):
        assert rel_l2(got.grad.cpu(), r.grad) < 1e-6
    for got in (Lp_d, Lq_d):          # gradient of a log-determinant: the diagonal only, exact zeros elsewhere
        off = got.grad - torch.diag_embed(got.grad.diagonal(dim1=-2, dim2=-1))
        assert torch.equal(off, torch.zeros_like(off))


# ---- variational hyper-parameters -----------------------------------------------------------------------------
@pytest.mark.parametrize('S', [1, 3, 64])
@pytest.mark.parametrize('D1', [3, 256, 257, 785])
def test_hyper_sample_and_kl_edges(ops, D1, S):
    """hyper_sample (one thread per sample entry, per-d reduction over S) and hyper_kl (ONE 256-thread block looping over D + 1:
    257 and 785 take more than one pass) against orc.sample_hypers / orc.kl_hypers in fp64."""
    mean = _hn((D1,), 800 + D1)
    logvar = _hu((D1,), 801 + D1, -4.0, 2.0)
    pmean, plogvar = _hn((D1,), 802 + D1, 0.5), _hn((D1,), 803 + D1, 0.5)
    eps = _hn((S, D1), 804 + D1 + S)
    m_d, v_d = mean.to(DEV).requires_grad_(True), logvar.to(DEV).requires_grad_(True)
    theta = ops.hyper_sample(m_d, v_d, eps.to(DEV))
    kl = ops.hyper_kl(m_d, v_d, pmean.to(DEV), plogvar.to(DEV))
    wt = _hn((S, D1), 805 + D1)
    ((theta * wt.to(DEV)).sum() + 2.5 * kl).backward()

    m64, v64 = _d64(mean), _d64(logvar)
    th64 = orc.sample_hypers(m64, v64, eps.double())
    kl64 = orc.kl_hypers(m64, v64, pmean.double(), plogvar.double())
    ((th64 * wt.double()).sum() + 2.5 * kl64).backward()
    assert rel_l2(theta.detach().cpu(), th64.detach()) < 1e-6
    assert abs(kl.item() - kl64.item()) <= 2e-6 * abs(kl64.item()), (kl.item(), kl64.item())
    assert rel_l2(m_d.grad.cpu(), m64.grad) < 2e-6
    assert rel_l2(v_d.grad.cpu(), v64.grad) < 2e-6
    # the two backward kernels on their own: a gradient into the sample only, and into the KL only
    for which in ('sample', 'kl'):
        m_d.grad = v_d.grad = None
        m64.grad = v64.grad = None
        if which == 'sample':
            (ops.hyper_sample(m_d, v_d, eps.to(DEV)) * wt.to(DEV)).sum().backward()
            (orc.sample_hypers(m64, v64, eps.double()) * wt.double()).sum().backward()
        else:
            (1.5 * ops.hyper_kl(m_d, v_d, pmean.to(DEV), plogvar.to(DEV))).backward()
            (1.5 * orc.kl_hypers(m64, v64, pmean.double(), plogvar.double())).backward()
        assert rel_l2(m_d.grad.cpu(), m64.grad) < 2e-6, which
        assert rel_l2(v_d.grad.cpu(), v64.grad) < 2e-6, which


# ---- packed triangle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m', [1, 2, 63, 64, 65, 100, 257])
def test_vec2tril_softplus_threshold(ops, m):
    """vec2tril / its backward / mat2trilvec against orc.vec2tril in fp64, with diagonal entries on both sides of the softplus
    threshold (19.9, 20.0: log1p(exp(x)); 20.1: x itself; -30: exp(x)) -- the backward is sigmoid(x) or 1 there, compared
    entry by entry."""
    nb = 3
    n = m * (m + 1) // 2
    vec = _hn((nb, n), 900 + m, 3.0)
    special = torch.tensor([19.9, 20.0, 20.1, -30.0])
    diag_idx = torch.arange(m) * (torch.arange(m) + 3) // 2            # packed index of (i, i): i (i + 1) / 2 + i
    for b in range(nb):
        k = min(m, 4)
        vec[b, diag_idx[:k]] = special.roll(b)[:k]
    v_d = vec.to(DEV).requires_grad_(True)
    L = ops.vec2tril(v_d, m)
    w = _hn(L.shape, 901 + m)
    (L * w.to(DEV)).sum().backward()
    v64 = _d64(vec)
    L64 = orc.vec2tril(v64, m)
    (L64 * w.double()).sum().backward()
    np.testing.assert_allclose(L.detach().cpu().double().numpy(), L64.detach().numpy(), rtol=1e-6, atol=0)
    assert torch.equal(L.detach().triu(1), torch.zeros_like(L))
    # every packed entry gets its gradient: g (strictly lower) or g * softplus'(x) (diagonal), relative to itself
    np.testing.assert_allclose(v_d.grad.cpu().double().numpy(), v64.grad.numpy(), rtol=1e-6, atol=0)
    back = ops.mat2trilvec(L.detach())
    assert torch.equal(back.cpu(), orc.mat2trilvec(L.detach().cpu()))


# ---- triangular solve through the inverse factor --------------------------------------------------------------
@pytest.mark.parametrize('nrhs', [1, 45, 512])
@pytest.mark.parametrize('n', [1, 64, 100, 101, 200])
def test_trsm_lower_edges(ops, n, nrhs):
    nb = 2
    A = _hn((nb, n, n), 1000 + n)
    A = A @ A.mT / n + torch.eye(n)
    B = _hn((nb, n, nrhs), 1001 + nrhs)
    gX = _hn((nb, n, nrhs), 1002 + nrhs)
    with torch.no_grad():
        L, T = ops.chol_inv(A.to(DEV), 0.0)
    Ld, Bd = L.requires_grad_(True), B.to(DEV).requires_grad_(True)
    X = ops.trsm_lower(Ld, T, Bd)
    (X * gX.to(DEV)).sum().backward()
    L6, B6 = _d64(L), B.double().requires_grad_(True)
    X6 = torch.linalg.solve_triangular(L6, B6, upper=False)
    (X6 * gX.double()).sum().backward()
    assert rel_l2(X.detach().cpu(), X6.detach()) < 1e-5
    assert rel_l2(Bd.grad.cpu(), B6.grad) < 1e-5
    assert rel_l2(Ld.grad.cpu(), L6.grad.tril()) < 1e-5
    assert torch.equal(Ld.grad.triu(1), torch.zeros_like(Ld.grad))


# ---- deep-kernel feature map: Linear + bias (+ ReLU) ----------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('cols', [1, 64, 65, 300])
@pytest.mark.parametrize('rows', [1, 64, 65, 1000])
def test_linear_act_edges(ops, rows, cols, relu):
    """linear_act (MFMA GEMM + bias_act_fwd / _bwd): ragged 64-column blocks and 64-row groups of the backward.  Inputs on a
    grid of quarters, so that the pre-activation is exact in fp32 and in fp64 alike and the ReLU mask is the same on both
    sides; every 7th row of x and every 5th bias entry are 0, so pre-activations of exactly 0 occur (torch's ReLU gradient
    there: 0)."""
    K = 33
    x = (torch.round(4.0 * orc.hash_normal((rows, K), 1100 + rows)) / 4.0).float()
    x[torch.arange(rows) % 7 == 3] = 0.0
    Wt = (torch.round(2.0 * orc.hash_normal((cols, K), 1101 + cols)) / 4.0).float()
    b = (torch.round(4.0 * orc.hash_normal((cols,), 1102 + cols)) / 4.0).float()
    b[torch.arange(cols) % 5 == 2] = 0.0
    gy = _hn((rows, cols), 1103 + rows + cols)
    xd, Wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, Wt, b))
    y = ops.linear_act(xd, Wd, bd, relu)
    (y * gy.to(DEV)).sum().backward()
    x6, W6, b6 = (t.double().requires_grad_(True) for t in (x, Wt, b))
    h6 = x6 @ W6.T + b6
    y6 = torch.relu(h6) if relu else h6
    (y6 * gy.double()).sum().backward()
    if relu:
        assert bool(((h6 == 0) & (gy != 0)).any()) or rows == 1
    assert torch.equal(y.detach().cpu().double(), y6.detach())
    assert rel_l2(xd.grad.cpu(), x6.grad) < 1e-6
    assert rel_l2(Wd.grad.cpu(), W6.grad) < 1e-6
    assert rel_l2(bd.grad.cpu(), b6.grad) < 1e-6


# ---- broadcast reduction of matmul gradients (vargp_sum_outer) ------------------------------------------------
@pytest.mark.parametrize('lead', [1, 3, 64])
def test_matmul_broadcast_reduction(ops, lead):
    """A (lead, 4, 100, 300) @ B (4, 300, 80) + D (1, 4, 100, 80): the gradients of B and D are summed over the broadcast
    leading batch by vargp_sum_outer (ops._reduce_to), 96000 and 32000 entries per slice."""
    A = _hn((lead, 4, 100, 300), 1200 + lead).to(DEV).requires_grad_(True)
    B = _hn((4, 300, 80), 1201).to(DEV).requires_grad_(True)
    D = _hn((1, 4, 100, 80), 1202).to(DEV).requires_grad_(True)
    out = ops.matmul(A, B, D=D, alpha=0.5, beta=-2.0)
    w = _hn(out.shape, 1203 + lead)
    (out * w.to(DEV)).sum().backward()
    A64, B64, D64 = (_d64(t) for t in (A, B, D))
    ref = 0.5 * (A64 @ B64) - 2.0 * D64
    (ref * w.double()).sum().backward()
    assert rel_l2(out.detach().cpu(), ref.detach()) < 2e-6
    assert rel_l2(A.grad.cpu(), A64.grad) < 2e-6
    assert rel_l2(B.grad.cpu(), B64.grad) < 5e-6
    assert rel_l2(D.grad.cpu(), D64.grad) < 2e-6
