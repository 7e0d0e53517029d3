"""k-means on the device: ops.kmeans_assign / ops.kmeans_update (csrc/kmeans.hip), init.lloyd / init.kmeans_inducing and the
z_init='kmeans' / lengthscale_init='median' routes of the factories, against the fp64 restatement of tests/test_kmeans.py.

Rule (tests/sweep_rule.py), per case:  err(HIP, fp64) <= RTOL_SCALAR + 2 err(torch fp32 on the host, fp64).  For distances err is
the maximum over points of |d - d64| / (|x|^2 + |z|^2), d64 the fp64 distance to the centre the device chose, and the fp32 host
value is the inner-product form |x|^2 + |z|^2 - 2 x.z at the same entries, on one thread (as _one_thread in
tests/test_hip_predict_f.py).  For centres err is the relative L2 norm, the fp32 host value index_add_ and a divide.
A label is right when the fp64 distance to its centre is within 2 e_n of the fp64 minimum, e_n = the case's bound x the scale
|x_n|^2 + max(|z_label|^2, |z_best|^2): an argmin over values each wrong by at most e picks a centre at most 2 e from the best."""
import itertools

import pytest
import torch

from helpers import RTOL_SCALAR
from test_kmeans import ref_assign, ref_lloyd, ref_update

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DS = (1, 2, 32, 33, 40, 784)


def _one_thread(fn):
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(n)


def _d64(x, z):
    """fp64 squared distances (G, N, K), formed directly, one set at a time."""
    x, z = x.double(), z.double()
    return torch.stack([((x[:, None, :] - zg[None, :, :]) ** 2).sum(-1) for zg in z])


def _d32_inner(x, z):
    """the fp32 inner-product form (G, N, K)."""
    nx, nz = (x * x).sum(-1), (z * z).sum(-1)
    return nx[None, :, None] + nz[:, None, :] - 2.0 * (x @ z.mT)


def _case_data(G, N, K, D, seed):
    """randn points; every other centre (as far as there are points) is a copy of a data point, the rest are randn.
    -> (x, z, copies: list of (g, k, n) with z[g, k] == x[n] bitwise)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, D, generator=gen)
    z = torch.randn(G, K, D, generator=gen)
    copies = []
    for g in range(G):
        perm = torch.randperm(N, generator=gen)
        for k in range(0, min(K, N), 2):
            z[g, k] = x[perm[k]]
            copies.append((g, k, int(perm[k])))
    return x, z, copies


def _check_assign(x, z, tag, copies=()):
    """-> list of failure messages of one assign case (items 5 and 6), and prints its figures."""
    from vargp_amd import ops
    G, K, D = z.shape
    N = x.shape[0]
    label, dist2 = ops.kmeans_assign(x.to(DEV), z.to(DEV))
    assert label.shape == (G, N) and label.dtype == torch.int32 and dist2.shape == (G, N) and dist2.dtype == torch.float32
    label, dist2 = label.cpu().long(), dist2.cpu()
    msgs = []
    if not bool(((label >= 0) & (label < K)).all()):
        return [f'{tag}: labels outside [0, {K})']
    d64 = _d64(x, z)
    d32 = _one_thread(lambda: _d32_inner(x, z))
    nx, nz = (x.double() ** 2).sum(-1), (z.double() ** 2).sum(-1)                 # (N,), (G, K)
    at = lambda d: d.gather(-1, label.unsqueeze(-1)).squeeze(-1)                   # the entries (g, n, label[g, n])
    scale = nx[None, :] + nz.gather(-1, label)
    e_hip = ((dist2.double() - at(d64)).abs() / scale).max().item()
    e_32 = ((at(d32).double() - at(d64)).abs() / scale).max().item()
    bound = RTOL_SCALAR + 2.0 * e_32
    print(f'{tag}: dist err {e_hip:.2e} (fp32 host {e_32:.2e})', end='')
    if not e_hip <= bound:
        msgs.append(f'{tag}: dist err {e_hip:.2e} > {RTOL_SCALAR:.0e} + 2 x {e_32:.2e}')
    if not bool((dist2 >= 0).all()):
        msgs.append(f'{tag}: negative distance')
    # labels: no label is exempt
    best, kbest = d64.min(-1)
    e_n = bound * (nx[None, :] + torch.maximum(nz.gather(-1, label), nz.gather(-1, kbest)))
    gap = at(d64) - best
    print(f', worst label gap {(gap / e_n).max().item():.2e} of 2 e_n allowed 2', flush=True)
    if not bool((gap <= 2.0 * e_n).all()):
        msgs.append(f'{tag}: {int((gap > 2.0 * e_n).sum())} labels further than 2 e_n from the nearest centre')
    if D <= 32:
        for g, k, n in copies:
            if dist2[g, n].item() != 0.0 or label[g, n].item() != k:
                msgs.append(f'{tag}: point {n} coincides with centre {k} of set {g}: label {label[g, n].item()}, '
                            f'dist2 {dist2[g, n].item()!r}')
                break
    return msgs


SMALL = [(1 + 2 * (i % 2), N, K, DS[i % 6]) for i, (N, K) in enumerate(itertools.product((1, 63, 65, 130), (1, 5, 33, 65)))]
FULL = [(G, 257, 130, D) for D, G in zip(DS, (1, 3, 1, 3, 3, 1))]


def test_assign_sweep():
    """22 cases: every D of (1, 2, 32, 33, 40, 784) at N = 257, K = 130 (five point tiles of 64, three centre tiles, both ragged) and
    the 16 pairs of N in (1, 63, 65, 130) with K in (1, 5, 33, 65), D and G in {1, 3} cycling through them."""
    bad = []
    for i, (G, N, K, D) in enumerate(FULL + SMALL):
        x, z, copies = _case_data(G, N, K, D, seed=100 + i)
        bad += _check_assign(x, z, f'G{G} N{N} K{K} D{D}', copies)
    assert not bad, bad


@pytest.mark.parametrize('K,D', [(130, 33), (5, 2)])
def test_assign_large_tile(K, D):
    """N G above 32768 takes the 128-point tiles (csrc/kmeans.hip: kKmSmallNG): N = 11000, G = 3 is 86 tiles per set, the last one
    ragged; K = 130 is two centre tiles of 128."""
    x, z, copies = _case_data(3, 11000, K, D, seed=7 + D)
    msgs = _check_assign(x, z, f'G3 N11000 K{K} D{D}', copies)
    assert not msgs, msgs


def _blobs(G, N, K, D, seed):
    """K well-separated blobs (spacing >= 10, spread 0.1), point n in blob n % K; per set the true centres in another order,
    slightly moved.  -> (x, z, blob of each point, order (G, K): z[g, k] is near the centre of blob order[g, k])"""
    gen = torch.Generator().manual_seed(seed)
    if D == 2:
        k = torch.arange(K)
        centres = torch.stack([10.0 * (k % 12), 10.0 * (k // 12)], -1).float()
    else:
        centres = 10.0 * torch.randn(K, D, generator=gen)
    blob = torch.arange(N) % K
    x = centres[blob] + 0.1 * torch.randn(N, D, generator=gen)
    order = torch.stack([torch.randperm(K, generator=gen) for _ in range(G)])
    z = centres[order] + 0.05 * torch.randn(G, K, D, generator=gen)
    return x, z, blob, order


@pytest.mark.parametrize('D', [2, 40])
def test_assign_blobs_exact_labels(D):
    from vargp_amd import ops
    G, N, K = 3, 257, 130
    x, z, blob, order = _blobs(G, N, K, D, seed=D)
    label = ops.kmeans_assign(x.to(DEV), z.to(DEV))[0].cpu().long()
    want = ref_assign(x.double(), z.double())[0]
    assert torch.equal(want, torch.argsort(order, -1)[:, blob])                  # the fp64 labels are the blobs
    assert torch.equal(label, want)
    assert not _check_assign(x, z, f'blobs D{D}')


@pytest.mark.parametrize('D', [2, 40])
def test_assign_ties_go_to_the_smallest_index(D):
    """Rows k = 3 and k = 70 of every set are bitwise the same (two centre tiles of 64 apart) and a data point: that point, and
    whoever else is nearest to them, gets label 3, nobody 70 -- in the direct form (D = 2) and in the MFMA form (D = 40)."""
    from vargp_amd import ops
    G, N, K = 3, 257, 130
    gen = torch.Generator().manual_seed(31 + D)
    x, z = torch.randn(N, D, generator=gen), torch.randn(G, K, D, generator=gen)
    rows = [11, 100, 256]
    for g in range(G):
        z[g, 3] = x[rows[g]]
        z[g, 70] = z[g, 3]
    label = ops.kmeans_assign(x.to(DEV), z.to(DEV))[0].cpu().long()
    assert not bool((label == 70).any())
    want = ref_assign(x.double(), z.double())[0]
    for g in range(G):
        assert want[g, rows[g]].item() == 3 and label[g, rows[g]].item() == 3
    assert not _check_assign(x, z, f'ties D{D}')


# -- update -------------------------------------------------------------------------------------------------------------------------
def _rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


UPDATE_CASES = [(3, 257, 130, 40), (1, 300, 1, 784), (2, 5, 33, 2), (1, 5000, 1, 40), (3, 5000, 7, 33), (1, 70, 3, 1100)]


@pytest.mark.parametrize('G,N,K,D', UPDATE_CASES)
def test_update(G, N, K, D):
    """Given the fp64 labels: the centres by the rule in relative L2, exact counts, a centre nobody chose bitwise unchanged with
    count 0, two calls bitwise equal.  K = 1: one cluster holds all the points (N = 5000: the index list in LDS is flushed
    inside the loop); N = 5 < K = 33: most centres are empty; D = 1100: two slabs of d."""
    from vargp_amd import ops
    x, z, _ = _case_data(G, N, K, D, seed=500 + N + K)
    label = ref_assign(x.double(), z.double())[0]
    z64, count64 = ref_update(x.double(), label, z.double())

    def host32():
        out = torch.zeros(G, K, D)
        for g in range(G):
            out[g].index_add_(0, label[g], x)
        cnt = count64.float().unsqueeze(-1)
        return torch.where(cnt > 0, out / cnt.clamp_min(1.0), z)
    z32 = _one_thread(host32)
    xd, ld, zd = x.to(DEV), label.to(DEV, torch.int32), z.to(DEV)
    z_new, count = ops.kmeans_update(xd, ld, zd)
    z_again, count_again = ops.kmeans_update(xd, ld, zd)
    assert torch.equal(zd.cpu(), z)                                           # the input is not modified
    assert z_new.shape == (G, K, D) and count.dtype == torch.int32
    assert torch.equal(z_new, z_again) and torch.equal(count, count_again)
    assert torch.equal(count.cpu().long(), count64)
    empty = count64 == 0
    assert torch.equal(z_new.cpu()[empty], z[empty])
    if K > N:
        assert bool(empty.any())
    e_hip, e_32 = _rel_l2(z_new.cpu(), z64), _rel_l2(z32, z64)
    print(f'G{G} N{N} K{K} D{D}: centres err {e_hip:.2e} (fp32 host {e_32:.2e})')
    assert e_hip <= RTOL_SCALAR + 2.0 * e_32, (e_hip, e_32)


# -- lloyd --------------------------------------------------------------------------------------------------------------------------
EPS32 = 2.0 ** -23


def _inertia_slack(x, z, label):
    """How far the inertia lloyd reports (the sum of the device's fp32 distances) may lie from the fp64 inertia of the same centres
    and labels, (G,).  For D > 32 a distance is |x|^2 + |z|^2 - 2 x.z, three fp32 sums of D terms each and two more roundings, so its
    forward error is at most (D + 3) eps (|x|^2 + |z|^2 + 2 |x| |z|) <= 2 (D + 3) eps (|x|^2 + |z|^2): an error relative to the
    SCALE of item 5, not to the distance, which for points far from the origin and near their centre is orders of magnitude
    smaller (blobs at |x|^2 = 4000 with d2 = 0.4).  The direct form (D <= 32) is inside the same bound."""
    D = x.shape[1]
    nx, nz = (x.double() ** 2).sum(-1), (z.double() ** 2).sum(-1)
    return (2.0 * (D + 3) * EPS32 * (nx[None, :] + nz.gather(-1, label))).sum(-1)


def test_lloyd_from_one_seed_per_blob():
    from vargp_amd import init
    G, N, K, D = 2, 257, 6, 40
    x, _, blob, order = _blobs(G, N, K, D, seed=3)
    first = torch.stack([torch.stack([x[(blob == b).nonzero()[0, 0]] for b in order[g]]) for g in range(G)])     # a point of each blob
    z64, label64, inertia64, n64 = ref_lloyd(x.double(), first.double(), 10)
    means = torch.stack([torch.stack([x.double()[blob == b].mean(0) for b in order[g]]) for g in range(G)])
    assert torch.allclose(z64, means, rtol=0, atol=1e-12) and n64 == 1
    z, label, inertia, n_done = init.lloyd(x.to(DEV), first.to(DEV), 10)
    assert n_done <= 3 and n_done == n64                 # the means after one update, confirmed by the assign that follows it
    assert torch.equal(label.cpu().long(), label64)
    z32 = _one_thread(lambda: torch.stack([torch.zeros(K, D).index_add_(0, label64[g], x) for g in range(G)])
                      / torch.stack([torch.bincount(label64[g], minlength=K) for g in range(G)]).float().unsqueeze(-1))
    e_hip, e_32 = _rel_l2(z.cpu(), z64), _rel_l2(z32, z64)
    print(f'blob means: err {e_hip:.2e} (fp32 host {e_32:.2e}); inertia {inertia.tolist()} vs {inertia64.tolist()}')
    assert e_hip <= RTOL_SCALAR + 2.0 * e_32
    slack = _inertia_slack(x, z64, label64)
    print(f'inertia off by {(inertia.cpu() - inertia64).abs().tolist()}, fp32 forward-error bound {slack.tolist()}')
    assert inertia.dtype == torch.float64 and bool(((inertia.cpu() - inertia64).abs() <= slack).all())


def test_lloyd_from_random_seeds_never_gets_worse():
    """The fp64 inertia of successive iterates (recomputed on the host from the returned centres) never rises by more than
    sum_n 2 e_n, e_n = RTOL_SCALAR x (|x_n|^2 + max_k |z_k|^2) -- the rule's bound without its fp32 term, so no wider."""
    from vargp_amd import init
    G, N, K, D = 3, 600, 9, 40
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, D, generator=gen) + 3.0 * torch.randn(6, D, generator=gen)[torch.arange(N) % 6]
    z0 = torch.stack([x[torch.randperm(N, generator=gen)[:K]] for _ in range(G)])
    xd, z0d = x.to(DEV), z0.to(DEV)
    nx = (x.double() ** 2).sum(-1)
    zs = [init.lloyd(xd, z0d, t) for t in range(7)]
    assert zs[0][0] is z0d and zs[0][3] == 0 and torch.equal(zs[0][0].cpu(), z0)
    inert = []
    for z, label, inertia, n_done in zs:
        d64 = _d64(x, z.cpu())
        inert.append(d64.min(-1).values.sum(-1))
        # what lloyd reports belongs to the centres and labels it returns (fp32 forward-error bound of the distances)
        own = d64.gather(-1, label.cpu().long().unsqueeze(-1)).squeeze(-1).sum(-1)
        assert bool(((inertia.cpu() - own).abs() <= _inertia_slack(x, z.cpu(), label.cpu().long())).all()), (inertia, own)
    print('fp64 inertia per iterate:', [[round(v, 3) for v in i.tolist()] for i in inert])
    for t in range(1, 7):
        nz = (zs[t][0].cpu().double() ** 2).sum(-1).max(-1).values                       # (G,)
        slack = (2.0 * RTOL_SCALAR * (nx[None, :] + nz[:, None])).sum(-1)
        assert bool((inert[t] <= inert[t - 1] + slack).all()), (t, inert[t - 1], inert[t])
    assert bool((inert[6] < inert[0]).all())


def test_kmeans_inducing_zero_iterations_is_the_random_route():
    from vargp_amd import init
    N, M, C = 200, 7, 3
    x = torch.randn(N, 40, generator=torch.Generator().manual_seed(9))
    torch.manual_seed(4)
    want = torch.stack([x[torch.randperm(N)[:M]] for _ in range(C)])
    torch.manual_seed(4)
    got = init.kmeans_inducing(x.to(DEV), C, M, n_iter=0)
    assert torch.equal(got.cpu(), want)


# -- the factories ------------------------------------------------------------------------------------------------------------------
class _Data:
    def __init__(self, x, targets):
        self.x, self.targets = x, targets

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.targets[i]


@pytest.mark.parametrize('which', ['clf', 'reg'])
def test_factories_kmeans_and_median(which):
    from vargp_amd import ops
    from vargp_amd.vargp import VARGP
    N, D, M = 600, 40, 6
    gen = torch.Generator().manual_seed(12)
    blob = torch.arange(N) % 6
    x = (3.0 * torch.randn(6, D, generator=gen))[blob] + 0.3 * torch.randn(N, D, generator=gen)
    if which == 'clf':
        data, make, C = _Data(x, blob), VARGP.create_clf, 6
        y = blob[:64]
    else:
        t = torch.stack([x[:, 0] + 0.1 * torch.randn(N, generator=gen), x[:, 1] - x[:, 2]], -1)
        data, make, C = _Data(x, t), VARGP.create_reg, 2
        y = t[:64].t().contiguous()
    torch.manual_seed(0)
    ref = make(data, M=M)
    torch.manual_seed(0)
    gp = make(data, M=M, z_init='kmeans', lengthscale_init='median')
    assert gp.z.shape == ref.z.shape == (C, M, D) and gp.z.dtype == ref.z.dtype and gp.z.device == ref.z.device
    xd = x.to(DEV)
    inertia = lambda z: ops.kmeans_assign(xd, z.detach().to(DEV))[1].double().sum(-1)
    i_seed, i_km = inertia(ref.z), inertia(gp.z)
    print(f'{which}: inertia of the seeds {i_seed.tolist()}, of the k-means centres {i_km.tolist()}')
    assert bool((i_km <= i_seed).all()) and bool((i_km < i_seed).any())
    ell = gp.kernel.log_mean.detach()[:-1].exp()
    assert bool((ell == ell[0]).all()) and 1.0 < ell[0].item() < 100.0
    gp = gp.to(DEV)
    kl_h, kl_u, nll = gp.loss(xd[:64], y.to(DEV))
    (kl_h + kl_u + nll).backward()
    for v in (kl_h, kl_u, nll):
        assert torch.isfinite(v).all()
    for name, p in gp.named_parameters():
        if p.grad is not None:
            assert torch.isfinite(p.grad).all(), name
    assert gp.z.grad is not None and gp.kernel.log_mean.grad is not None
