"""Data-dependent initialisation, the part that needs no GPU: the fp64 restatement of k-means that tests/test_hip_kmeans.py
measures the device against (ref_assign / ref_update / ref_lloyd, checked here on hand-computable cases), init.median_lengthscale
and RBFKernel.set_lengthscale_, the workspace query of csrc/kmeans.hip, the argument checks of its three C-ABI entries and of
the factories, and the promise that the default arguments change nothing."""
import ctypes
import math

import pytest
import torch

from vargp_amd import init
from vargp_amd.kernels import DeepRBFKernel, MaternKernel, RBFKernel
from vargp_amd.vargp import VARGP


# -- the fp64 restatement -----------------------------------------------------------------------------------------------------------
def ref_dist2(x, z):
    """x (N, D), z (G, K, D) -> squared Euclidean distances (G, N, K), formed directly, in the dtype of the inputs."""
    return ((x[None, :, None, :] - z[:, None, :, :]) ** 2).sum(-1)


def ref_assign(x, z):
    """-> (label int64 (G, N): the nearest centre, the smallest index on a tie; dist2 (G, N))."""
    d2 = ref_dist2(x, z)
    m = d2.min(-1).values
    K = z.shape[1]
    label = torch.where(d2 == m.unsqueeze(-1), torch.arange(K).expand_as(d2), torch.full_like(d2, K, dtype=torch.int64)).min(-1).values
    return label, m


def ref_update(x, label, z):
    """-> (z_new (G, K, D): the mean of each label's points, a centre without points kept as it is; count int64 (G, K))."""
    G, K, _ = z.shape
    z_new, count = z.clone(), torch.zeros(G, K, dtype=torch.int64)
    for g in range(G):
        for k in range(K):
            mask = label[g] == k
            count[g, k] = int(mask.sum())
            if count[g, k]:
                z_new[g, k] = x[mask].mean(0)
    return z_new, count


def ref_lloyd(x, z0, n_iter):
    """vargp_amd.init.lloyd, restated: -> (z, label, inertia (G,), n_done)."""
    z = z0
    label, d2 = ref_assign(x, z)
    n_done = 0
    for _ in range(n_iter):
        z, _ = ref_update(x, label, z)
        new_label, d2 = ref_assign(x, z)
        n_done += 1
        same = torch.equal(new_label, label)
        label = new_label
        if same:
            break
    return z, label, d2.sum(-1), n_done


BLOB_CENTRES = torch.tensor([[10.0, 10.0], [-10.0, 10.0], [-10.0, -10.0], [10.0, -10.0]], dtype=torch.float64)
BLOB_OFFSETS = torch.tensor([[0.5, 0.0], [-0.5, 0.0], [0.0, 0.75], [0.0, 0.25]], dtype=torch.float64)      # mean (0, 0.25)


def four_blobs():
    """16 points in D = 2: four per blob, blob b at rows b, b + 4, b + 8, b + 12; the blob means are BLOB_CENTRES + (0, 0.25),
    and the inertia about them is 4 x (0.3125 + 0.3125 + 0.25 + 0) = 3.5."""
    x = (BLOB_CENTRES[None, :, :] + BLOB_OFFSETS[:, None, :]).reshape(16, 2)
    return x, torch.arange(16) % 4


def test_ref_four_blobs():
    x, blob = four_blobs()
    # one seed per blob (its first point), in the order 2, 0, 3, 1 of the blobs
    order = torch.tensor([2, 0, 3, 1])
    z0 = x[order].unsqueeze(0)
    label, d2 = ref_assign(x, z0)
    want = torch.argsort(order)[blob]
    assert torch.equal(label[0], want)
    assert d2[0, order[0]].item() == 0.0                                   # a seed is its own nearest centre
    z, label, inertia, n_done = ref_lloyd(x, z0, 10)
    assert n_done == 1 and torch.equal(label[0], want)
    assert torch.allclose(z[0], BLOB_CENTRES[order] + torch.tensor([0.0, 0.25], dtype=torch.float64), rtol=0, atol=1e-14)
    assert abs(inertia.item() - 3.5) < 1e-12
    z_again, _, _, n0 = ref_lloyd(x, z0, 0)
    assert z_again is z0 and n0 == 0


def test_ref_duplicate_and_empty_centres():
    x, blob = four_blobs()
    far = torch.tensor([[500.0, 500.0]], dtype=torch.float64)
    # centres: blob 0's mean, blob 1's mean, blob 0's mean AGAIN (k = 2), a centre nobody is near (k = 3)
    m = BLOB_CENTRES + torch.tensor([0.0, 0.25], dtype=torch.float64)
    z = torch.cat([m[0:1], m[1:2], m[0:1], far]).unsqueeze(0)
    label, _ = ref_assign(x, z)
    assert set(label[0].tolist()) == {0, 1}                                # the tie between k = 0 and k = 2 goes to k = 0
    assert torch.equal(label[0][blob == 0], torch.zeros(4, dtype=torch.int64))
    z_new, count = ref_update(x, label, z)
    assert count[0].tolist() == [int((label[0] == 0).sum()), int((label[0] == 1).sum()), 0, 0] and count.sum() == 16
    assert torch.equal(z_new[0, 2], z[0, 2]) and torch.equal(z_new[0, 3], z[0, 3])          # kept, bit for bit
    # blobs 2 and 3 are split between the two live centres by distance: blob 3 (10, -10) is nearer to (10, 10.25)
    assert torch.equal(label[0][blob == 3], torch.zeros(4, dtype=torch.int64))
    assert torch.equal(label[0][blob == 2], torch.ones(4, dtype=torch.int64))
    assert torch.allclose(z_new[0, 0], x[(blob == 0) | (blob == 3)].mean(0))


# -- median_lengthscale -------------------------------------------------------------------------------------------------------------
# Relative spread of median_lengthscale over 4096 pairs, measured on the CPU with the function under test as the standard deviation
# over 20 seeds: 9.1e-4 on 0.7 randn(3000, 200) (mean 0.99931 of a sqrt(2 D): the median of chi2_200 lies 1 / (3 D) below D).  The
# chi-square form gives the same: d2 = 2 a^2 chi2_D has relative standard deviation sqrt(2 / D) = 0.1, its median over n pairs
# 1.2533 x 0.1 / sqrt(4096) = 2.0e-3, and the square root halves it: 9.8e-4.  The margin of every check below is 4 x the measured
# value.  On the unscaled MNIST surrogate the same measurement gives 5.2e-4 for the lengthscale and 6.2e-4 for the median kernel
# value at a fixed lengthscale (8.1e-4 together, inside the same margin).
SPREAD = 9.1e-4
MARGIN = 4 * SPREAD


def _surrogate(n=3000):
    from vargp_amd.synthetic import mnist_like
    return mnist_like(n, 784, 10, kind='mnist_classes', seed=0, sample_seed=1)[0]


def test_median_lengthscale_gaussian_and_scale():
    """a randn(N, D): sqrt(median |x_i - x_j|^2) = a sqrt(2 D) within 4 x the sampling spread of the median over
    4096 pairs (measured over 20 seeds: 9.1e-4 relative; 9.8e-4 from the chi-square form)."""
    a, N, D = 0.7, 3000, 200
    x = a * torch.randn(N, D, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(2)
    ell = init.median_lengthscale(x)
    assert abs(ell / (a * math.sqrt(2 * D)) - 1.0) <= MARGIN, ell
    torch.manual_seed(2)
    assert init.median_lengthscale(x, scale=2.5) == pytest.approx(2.5 * ell, rel=1e-12)
    torch.manual_seed(2)
    assert init.median_lengthscale(x, n_pairs=4096, scale=1.0) == ell
    with pytest.raises(ValueError):
        init.median_lengthscale(x[:1])


def _median_k(kern, x, seed):
    """median over 4096 random pairs of exp(-d2 / 2), d2 = sum_d ((x_i - x_j) / lengthscale_d)^2, in fp32 as the kernels form it."""
    g = torch.Generator().manual_seed(seed)
    N = x.shape[0]
    i = torch.randint(N, (4096,), generator=g)
    j = (i + torch.randint(1, N, (4096,), generator=g)) % N
    ls = kern.log_mean.detach()[:-1].exp()
    d2 = (((x[i] - x[j]) / ls) ** 2).sum(-1)
    return (-0.5 * d2).exp().median().item()


@pytest.mark.parametrize('cls', [RBFKernel, MaternKernel])
def test_median_lengthscale_on_the_unscaled_surrogate(cls):
    """The README's complaint, pinned: at pixel range [0, 1] (mnist_like WITHOUT datasets.kSyntheticScale) the default
    initialisation puts the median pair at a kernel value of exactly 0.0 in fp32; after set_lengthscale_(median_lengthscale(x))
    it is exp(-1/2) within the same margin (4 x 9.1e-4 relative), on pairs other than those the lengthscale came from."""
    x = _surrogate()
    torch.manual_seed(0)
    kern = cls(784)
    assert _median_k(kern, x, 5) == 0.0
    before = kern.log_mean.detach().clone(), kern.log_logvar.detach().clone()
    torch.manual_seed(3)
    ell = init.median_lengthscale(x)
    assert kern.set_lengthscale_(ell) is kern
    assert torch.equal(kern.log_mean.detach()[:-1], torch.full((784,), math.log(ell)))
    assert torch.equal(kern.log_mean.detach()[-1], before[0][-1]) and torch.equal(kern.log_logvar.detach(), before[1])
    assert kern.log_mean.requires_grad
    k = _median_k(kern, x, 5)
    assert abs(k / math.exp(-0.5) - 1.0) <= MARGIN, k
    with pytest.raises(ValueError):
        kern.set_lengthscale_(0.0)


def test_set_lengthscale_deep_kernel_sets_feature_lengthscales():
    torch.manual_seed(0)
    kern = DeepRBFKernel(10, feature_size=6)
    kern.set_lengthscale_(2.0)
    assert torch.equal(kern.log_mean.detach()[:-1], torch.full((6,), math.log(2.0)))


# -- the workspace query ------------------------------------------------------------------------------------------------------------
def test_workspace_never_holds_the_distance_matrix():
    from vargp_amd._lib import lib
    ws = lib().vargp_kmeans_workspace_bytes
    G, K, N, D = 10, 100, 60000, 784
    grow = ws(G, 200, N, D) - ws(G, K, N, D)
    assert grow == ws(G, 200, 2 * N, D) - ws(G, K, 2 * N, D)                       # what K costs does not depend on N
    assert 0 < ws(G, K, N, D) < 4 * (2 * N * D + 2 * G * K * D + 4 * N + 4 * G * K)
    assert ws(G, K, N, D) < 4 * N * K                                             # one set's N x K matrix alone is 24 MB
    assert ws(G, K, N, 2) > 0


# -- argument checks ----------------------------------------------------------------------------------------------------------------
def test_cabi_argument_errors_before_any_launch():
    """A null pointer, a zero size or a short workspace: VARGP_EINVAL (-1) from each entry, with host memory for pointers -- nothing
    is launched, so no device is touched."""
    from vargp_amd._lib import lib
    L = lib()
    EINVAL = -1
    G, K, N, D = 2, 3, 5, 40
    buf = (ctypes.c_float * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)
    need = L.vargp_kmeans_workspace_bytes(G, K, N, D)
    assert 0 < need <= 4096 * 4
    for fn in (L.vargp_kmeans_assign, L.vargp_kmeans_update):
        for bad in range(4):
            ptrs = [null if q == bad else p for q in range(4)]
            assert fn(*ptrs, G, K, N, D, p, need, None) == EINVAL
        assert fn(p, p, p, p, G, K, N, D, null, need, None) == EINVAL
        for dims in ((0, K, N, D), (G, 0, N, D), (G, K, 0, D), (G, K, N, 0), (-1, K, N, D)):
            assert fn(p, p, p, p, *dims, p, need, None) == EINVAL
        assert fn(p, p, p, p, G, K, N, D, p, need - 1, None) == EINVAL
        assert fn(p, p, p, p, G, K, N, D, p, 0, None) == EINVAL
        assert b'kmeans' in L.vargp_last_error()
    assert L.vargp_kmeans_workspace_bytes(0, K, N, D) == 0


def test_ops_refuse_cpu_tensors():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    x, z = torch.randn(6, 3), torch.randn(2, 2, 3)
    with pytest.raises(VargpHipError):
        ops.kmeans_assign(x, z)
    with pytest.raises(VargpHipError):
        ops.kmeans_update(x, torch.zeros(2, 6, dtype=torch.int32), z)
    with pytest.raises(VargpHipError):
        init.lloyd(x, z, 1)
    with pytest.raises(VargpHipError):
        init.kmeans_inducing(x, 2, 2)


class _Data:
    def __init__(self, x, targets):
        self.x, self.targets = x, targets

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.targets[i]


def _clf_data():
    g = torch.Generator().manual_seed(0)
    return _Data(torch.randn(60, 5, generator=g), torch.arange(60) % 3)


def _reg_data():
    g = torch.Generator().manual_seed(0)
    return _Data(torch.randn(60, 5, generator=g), torch.randn(60, 2, generator=g))


def test_factories_refuse_unknown_names():
    for make, data, who in ((VARGP.create_clf, _clf_data(), 'create_clf'), (VARGP.create_reg, _reg_data(), 'create_reg')):
        with pytest.raises(ValueError, match=who + ': z_init'):
            make(data, M=4, z_init='kmeans++')
        with pytest.raises(ValueError, match=who + ': lengthscale_init'):
            make(data, M=4, lengthscale_init='mean')
    with pytest.raises(ValueError, match='create_clf: lengthscale_init'):
        VARGP.create_clf(_clf_data(), M=4, dkl=True, lengthscale_init='median')


def test_default_arguments_change_nothing():
    """create_clf / create_reg with the default z_init and lengthscale_init: the parent commit's two lines, restated literally,
    give the same z bit for bit, and the kernel's own draws (which follow them on the global generator) are the same too."""
    for make, data, C in ((VARGP.create_clf, _clf_data(), 3), (VARGP.create_reg, _reg_data(), 2)):
        M = 7
        torch.manual_seed(0)
        gp = make(data, M=M)
        torch.manual_seed(0)
        N = len(data)
        z = torch.stack([data[torch.randperm(N)[:M]][0] for _ in range(C)])
        kern = RBFKernel(z.size(-1))
        assert gp.z.shape == (C, M, 5) and torch.equal(gp.z.detach(), z)
        assert torch.equal(gp.kernel.log_mean.detach(), kern.log_mean.detach())
        torch.manual_seed(0)
        gp2 = make(data, M=M, z_init='random', kmeans_iters=3, lengthscale_init='default')
        assert torch.equal(gp2.z.detach(), z) and torch.equal(gp2.kernel.log_mean.detach(), kern.log_mean.detach())


def test_median_init_through_the_factories():
    """lengthscale_init='median' needs no device: z and log gamma are those of the default route, every lengthscale is the
    median pair distance of the task's points; with previous tasks the handed-over hyper-posterior is the start, as before."""
    for make, data in ((VARGP.create_clf, _clf_data()), (VARGP.create_reg, _reg_data())):
        torch.manual_seed(0)
        ref = make(data, M=4)
        torch.manual_seed(0)
        gp = make(data, M=4, lengthscale_init='median')
        assert torch.equal(gp.z.detach(), ref.z.detach())
        lm = gp.kernel.log_mean.detach()
        assert torch.equal(lm[-1], ref.kernel.log_mean.detach()[-1])
        assert torch.equal(gp.kernel.log_logvar.detach(), ref.kernel.log_logvar.detach())
        ell = math.exp(lm[0].item())
        assert torch.equal(lm[:-1], lm[0].expand(5)) and abs(ell / math.sqrt(2 * 5) - 1.0) < 0.25      # randn data: about sqrt(2 D)
        # a second task: the lengthscales are NOT reset
        prev = [{k: v.detach().clone() for k, v in ref.state_dict().items()}]
        torch.manual_seed(1)
        a = make(data, M=4, prev_params=[dict(p) for p in prev])
        torch.manual_seed(1)
        b = make(data, M=4, prev_params=[dict(p) for p in prev], lengthscale_init='median')
        assert torch.equal(a.kernel.log_mean.detach(), b.kernel.log_mean.detach())
