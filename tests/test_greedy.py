"""Greedy conditional-variance selection of inducing points, the part that needs no GPU: the fp64 restatement that
tests/test_hip_greedy.py measures the device against (ref_greedy, checked here as the pivoted Cholesky it is and against random
subsets on clustered inputs), the workspace query and the argument checks of the C-ABI entry of csrc/greedy.hip, and the argument
checks of ops.greedy_select, init.greedy_inducing and the factories' z_init='greedy'."""
import ctypes
import math

import pytest
import torch

from vargp_amd import init
from vargp_amd.vargp import VARGP, _Z_INITS

JITTER = 1e-4


# -- the restatement ----------------------------------------------------------------------------------------------------------------
def ref_kernel(xa, xb, theta, nu2):
    """k(x, y) = gamma^2 f(r), r^2 = sum_d ((x_d - y_d) / lengthscale_d)^2, theta = [log lengthscale_1..D, log gamma]; xa (n, D)
    against xb (m, D) -> (n, m), in the dtype of the inputs.  nu2: 0 = RBF exp(-r^2 / 2); 1, 3, 5 = Matern nu = nu2 / 2."""
    ls, g2 = theta[:-1].exp(), (2.0 * theta[-1]).exp()
    r2 = (((xa[:, None, :] - xb[None, :, :]) / ls) ** 2).sum(-1)
    if nu2 == 0:
        return g2 * (-0.5 * r2).exp()
    a = (nu2 * r2).sqrt()
    poly = {1: 1.0, 3: 1.0 + a, 5: 1.0 + a + (5.0 / 3.0) * r2}[nu2]
    return g2 * poly * (-a).exp()


def ref_greedy(x, cand, theta, nu2, M, eps, LT0=None, d0=None, picks=None, dtype=torch.float64):
    """One candidate set: x (N, D), cand (Nc,) row numbers or None = all rows in order.  M steps of: key_i = d_i if d_i > eps else
    0 over the unselected candidates, p = the largest key (the lowest position on a tie) -- or picks[k] when picks is given --
    pivot[k] = d_p; if d_p > eps: c = k(x_cand, x_p) - LT[:r].T LT[:r, p], LT[r] = c / sqrt(d_p), d = max(d - LT[r]^2, 0), else
    LT[r] = 0 and d stays; p is selected.  r = k0 + k; LT0 (k0, Nc) and d0 (Nc,) start the factorisation, otherwise d = gamma^2.
    -> (pick int64 (M,), pivot (M,), LT (k0 + M, Nc), d (Nc,), d_before (M, Nc): d as each step found it)."""
    xc = (x if cand is None else x[cand]).to(dtype)
    theta = theta.to(dtype)
    Nc = xc.shape[0]
    k0 = 0 if LT0 is None else LT0.shape[0]
    LT = torch.zeros(k0 + M, Nc, dtype=dtype)
    if k0:
        LT[:k0] = LT0.to(dtype)
        d = d0.to(dtype).clone()
    else:
        d = (2.0 * theta[-1]).exp().expand(Nc).clone()
    selected = torch.zeros(Nc, dtype=torch.bool)
    pick, pivot, d_before = torch.zeros(M, dtype=torch.int64), torch.zeros(M, dtype=dtype), torch.zeros(M, Nc, dtype=dtype)
    for k in range(M):
        r = k0 + k
        d_before[k] = d
        if picks is None:
            key = torch.where(d > eps, d, torch.zeros_like(d))
            key[selected] = -1.0
            p = int((key == key.max()).nonzero()[0])
        else:
            p = int(picks[k])
        pick[k], pivot[k] = p, d[p]
        if d[p] > eps:
            c = ref_kernel(xc, xc[p:p + 1], theta, nu2)[:, 0] - LT[:r].T @ LT[:r, p]
            LT[r] = c / d[p].sqrt()
            d = (d - LT[r] ** 2).clamp_min(0.0)
        selected[p] = True
    return pick, pivot, LT, d, d_before


def ref_whitened_cross(theta, z, y, nu2, eps, dtype=torch.float64):
    """(T K(z, y), max(gamma^2 - colsum of its squares, 0)), T the inverse Cholesky factor of K(z, z) + eps I."""
    theta, z, y = theta.to(dtype), z.to(dtype), y.to(dtype)
    L = torch.linalg.cholesky(ref_kernel(z, z, theta, nu2) + eps * torch.eye(z.shape[0], dtype=dtype))
    A = torch.linalg.solve_triangular(L, ref_kernel(z, y, theta, nu2), upper=False)
    return A, ((2.0 * theta[-1]).exp() - (A * A).sum(0)).clamp_min(0.0)


def ref_residual(x, z, theta, nu2, eps=JITTER, dtype=torch.float64):
    """mean over the rows of x of gamma^2 - |T K(z, x)|^2 (init.nystrom_residual, restated), z (M, D)."""
    A, _ = ref_whitened_cross(theta, z, x, nu2, eps, dtype=dtype)
    return float(((2.0 * theta[-1].to(dtype)).exp() - (A * A).sum(0)).mean())


def clustered(N, D, seed):
    """Six Gaussian clusters of spread 0.3 with centres ~ 2 N(0, I), rows in random cluster order; float32 (N, D)."""
    g = torch.Generator().manual_seed(seed)
    centres = 2.0 * torch.randn(6, D, generator=g)
    return centres[torch.randint(6, (N,), generator=g)] + 0.3 * torch.randn(N, D, generator=g)


def median_theta(x, seed=0):
    """[log median-heuristic lengthscale] x D, log gamma = log 0.5 (gamma^2 = 0.25)."""
    torch.manual_seed(seed)
    ell = init.median_lengthscale(x)
    return torch.cat([torch.full((x.shape[1],), math.log(ell)), torch.tensor([math.log(0.5)])])


def random_subsets_residual(x, theta, nu2, M, n=20, seed=1, z_prev=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        z = x[torch.randperm(x.shape[0], generator=g)[:M]]
        out.append(ref_residual(x, z if z_prev is None else torch.cat([z_prev, z]), theta, nu2))
    return out


@pytest.mark.parametrize('nu2', [0, 1, 3, 5])
def test_ref_is_the_pivoted_cholesky(nu2):
    """M = Nc: LT^T LT = K(x, x) and nothing is left; every point is picked once; the pivots never grow; the first pick of an empty
    start is position 0, its pivot gamma^2 and its row K[0] / gamma."""
    x = clustered(9, 3, seed=3).double()
    theta = torch.tensor([0.1, -0.2, 0.3, math.log(0.7)], dtype=torch.float64)
    pick, pivot, LT, d, d_before = ref_greedy(x, None, theta, nu2, 9, 0.0)
    K = ref_kernel(x, x, theta, nu2)
    assert torch.allclose(LT.T @ LT, K, rtol=0, atol=1e-12)
    assert sorted(pick.tolist()) == list(range(9)) and pick[0] == 0
    assert float(d.max()) < 1e-12
    assert abs(float(pivot[0]) - 0.49) < 1e-15 and bool((pivot[1:] <= pivot[:-1] + 1e-15).all())
    assert torch.allclose(LT[0], K[0] / 0.7, rtol=0, atol=1e-15)
    assert torch.equal(d_before[0], torch.full((9,), 0.7 ** 2, dtype=torch.float64))
    # a subset of the rows in another order, and the same picks followed on request
    cand = torch.tensor([4, 2, 7, 0])
    a = ref_greedy(x, cand, theta, nu2, 3, 0.0)
    b = ref_greedy(x[cand], None, theta, nu2, 3, 0.0, picks=a[0])
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_ref_exhaustion_and_prefill():
    """5 distinct points repeated four times, M = 8: five picks of distinct points, then nothing is above eps: the lowest unselected
    positions, rows of zeros, d untouched.  And a factorisation started from the first three points (ref_whitened_cross with
    eps = 0) continues as the one that picked them itself."""
    base = clustered(5, 2, seed=5).double()
    x = base.repeat(4, 1)
    theta = torch.tensor([0.0, 0.0, 0.0], dtype=torch.float64)
    pick, pivot, LT, d, _ = ref_greedy(x, None, theta, 0, 8, JITTER)
    assert sorted((pick[:5] % 5).tolist()) == [0, 1, 2, 3, 4]
    assert bool((pivot[5:] <= JITTER).all()) and bool((pivot[:5] > JITTER).all())
    rest = [i for i in range(20) if i not in pick[:5].tolist()]
    assert pick[5:].tolist() == rest[:3]
    assert float(LT[5:].abs().max()) == 0.0
    full = ref_greedy(x[:5], None, theta, 0, 5, 0.0)
    LT0, d0 = ref_whitened_cross(theta, x[full[0][:3]], x[:5], 0, 0.0)
    cont = ref_greedy(x[:5], None, theta, 0, 2, 0.0, LT0=LT0, d0=d0, picks=full[0][3:])
    assert torch.allclose(cont[3], full[3], rtol=0, atol=1e-12) and torch.allclose(cont[1], full[1][3:], rtol=0, atol=1e-12)
    assert torch.allclose(cont[2][3:].abs(), full[2][3:].abs(), rtol=0, atol=1e-10)


@pytest.mark.parametrize('D', [5, 784])
@pytest.mark.parametrize('nu2', [0, 3])
def test_ref_beats_random_subsets_on_clusters(D, nu2):
    """Six clusters, median-heuristic lengthscale, gamma^2 = 0.25, N = 257, M = 24: the mean residual variance the greedy points
    leave is below the mean over 20 random M-subsets (not always below the best of them: not asserted)."""
    x = clustered(257, D, seed=11)
    theta = median_theta(x)
    pick = ref_greedy(x, None, theta, nu2, 24, JITTER)[0]
    greedy = ref_residual(x, x[pick], theta, nu2)
    rand = random_subsets_residual(x, theta, nu2, 24)
    print(f'D={D} nu2={nu2}: greedy {greedy:.4g}  random mean {sum(rand) / len(rand):.4g}  best {min(rand):.4g}')
    assert greedy < sum(rand) / len(rand)


# -- the workspace query ------------------------------------------------------------------------------------------------------------
def test_workspace_is_linear_in_the_candidates():
    from vargp_amd._lib import lib
    ws = lib().vargp_greedy_workspace_bytes
    G, D, Mtot = 10, 784, 500
    assert ws(0, 4096, D, Mtot) == 0
    step = ws(G, 8192, D, Mtot) - ws(G, 4096, D, Mtot)
    assert step > 0 and step == ws(G, 65536, D, Mtot) - ws(G, 61440, D, Mtot)      # the same 4096 candidates cost the same anywhere
    assert 0 < ws(G, 65536, D, Mtot) < 16 * G * 65536 + 4 * 65536                  # a few words per candidate, never Nc x Nc
    assert ws(1, 1, 1, 1) > 0


# -- argument checks ----------------------------------------------------------------------------------------------------------------
def test_cabi_argument_errors_before_any_launch():
    """A null pointer other than cand, a size < 1, k0 < 0, M > Nc, a kernel code outside the four, G > 65535 or a short workspace:
    VARGP_EINVAL (-1), with host memory for pointers -- nothing is launched, so no device is touched."""
    from vargp_amd._lib import lib
    L = lib()
    EINVAL = -1
    G, Nc, N, D, k0, M = 2, 6, 9, 40, 0, 3
    buf = (ctypes.c_float * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    null = ctypes.c_void_p(0)
    need = L.vargp_greedy_workspace_bytes(G, Nc, D, k0 + M)
    assert 0 < need <= 4096 * 4
    fn = L.vargp_greedy_select

    def call(ptrs=None, dims=(G, Nc, N, D, k0, M), nu2=0, ws=p, ws_bytes=need):
        return fn(*(ptrs or [p] * 7), *dims, nu2, JITTER, ws, ws_bytes, None)

    for bad in (0, 1, 3, 4, 5, 6):                                   # every pointer but cand (2)
        assert call([null if q == bad else p for q in range(7)]) == EINVAL
    assert call(ws=null) == EINVAL
    no_cand = [null if q == 2 else p for q in range(7)]
    assert call(no_cand, dims=(G, N + 1, N, D, k0, M), ws_bytes=1 << 40) == EINVAL       # rows 0..Nc-1 of an X with fewer rows
    for dims in ((0, Nc, N, D, k0, M), (G, 0, N, D, k0, 0), (G, Nc, 0, D, k0, M), (G, Nc, N, 0, k0, M), (G, Nc, N, D, k0, 0),
                 (-1, Nc, N, D, k0, M), (G, Nc, N, D, -1, M), (G, Nc, N, D, k0, Nc + 1), (65536, Nc, N, D, k0, M)):
        assert call(dims=dims, ws_bytes=1 << 40) == EINVAL, dims
    for nu2 in (-1, 2, 4, 6):
        assert call(nu2=nu2) == EINVAL
    assert call(ws_bytes=need - 1) == EINVAL and call(ws_bytes=0) == EINVAL
    assert b'greedy' in L.vargp_last_error()
    assert L.vargp_greedy_workspace_bytes(0, Nc, D, M) == 0


def test_ops_refuse_cpu_tensors():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    x, theta = torch.randn(6, 3), torch.zeros(4)
    with pytest.raises(VargpHipError):
        ops.greedy_select(theta, x, M=2)
    with pytest.raises(VargpHipError):
        ops.greedy_select(theta, x, torch.zeros(1, 4, dtype=torch.int32), M=2)
    with pytest.raises(VargpHipError):
        init.greedy_inducing(x, 2, 2, theta)
    with pytest.raises(VargpHipError):
        init.nystrom_residual(x, torch.randn(2, 2, 3), theta)


def test_draw_candidates_is_the_random_routes_draw():
    torch.manual_seed(4)
    cand = init.draw_candidates(11, 3, 5)
    torch.manual_seed(4)
    want = torch.stack([torch.randperm(11)[:5] for _ in range(3)])
    assert torch.equal(cand, want)
    assert init.draw_candidates(4, 2, 4096).shape == (2, 4)


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


def test_factories_accept_greedy_only_in_valid_combinations():
    """Refused before anything runs on a device: dkl (the features are untrained) and more inducing points than candidates."""
    assert 'greedy' in _Z_INITS
    with pytest.raises(ValueError, match="create_clf: z_init='greedy'"):
        VARGP.create_clf(_clf_data(), M=4, dkl=True, z_init='greedy')
    for make, data, who in ((VARGP.create_clf, _clf_data(), 'create_clf'), (VARGP.create_reg, _reg_data(), 'create_reg')):
        with pytest.raises(ValueError, match=who + ": z_init='greedy' picks M = 61"):
            make(data, M=61, z_init='greedy')
        with pytest.raises(ValueError, match=who + ": z_init='greedy' picks M = 8"):
            make(data, M=8, z_init='greedy', greedy_candidates=7)
        with pytest.raises(ValueError, match=who + ': z_init'):
            make(data, M=4, z_init='greedy++')


def test_driver_takes_the_new_arguments():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'experiments', 'vargp.py')
    spec = importlib.util.spec_from_file_location('vargp_driver_for_greedy', path)
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    args = drv.parse_args(['s_mnist', '--z_init', 'greedy', '--greedy_candidates', '512'])
    assert args.z_init == 'greedy' and args.greedy_candidates == 512
    assert drv.parse_args(['toy']).greedy_candidates == 4096 and drv.parse_args(['toy']).z_init == 'random'
