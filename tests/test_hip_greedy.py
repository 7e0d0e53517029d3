"""Greedy conditional-variance selection on the device: ops.greedy_select (csrc/greedy.hip), init.greedy_inducing /
init.nystrom_residual and the z_init='greedy' route of the factories, against the fp64 restatement of tests/test_greedy.py.

Rule (tests/sweep_rule.py), per case and set: the fp64 reference FOLLOWS the device's picks, so no case is exempt and no near-tie
needs special inputs.  e = (RTOL_SCALAR + 2 err32) gamma^2, err32 the worst |d32 - d64| / gamma^2 over all steps of the fp32 host
restatement on one thread along the same picks.  pivot[k], the final d: within e of fp64; the new row of LT: within
e / sqrt(pivot).  The pick, against the fp64 keys along the device's path: if the fp64 maximum is >= eps + 2 e, the device's pick
has an fp64 d within 2 e of it (an argmax over values each wrong by at most e); if it is <= eps - 2 e, the device's pick is the
lowest unselected position and its row is exactly zero; in between either is accepted."""
import math

import pytest
import torch

from helpers import RTOL_SCALAR
from test_greedy import (JITTER, clustered, median_theta, random_subsets_residual, ref_greedy, ref_residual, ref_whitened_cross)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _one_thread(fn):
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(n)


def _check(x, cand, theta, nu2, M, G, tag, eps=JITTER, LT0=None, d0=None):
    """Run ops.greedy_select and hold every set to the rule.  cand (G, Nc) int64 on the host or None; LT0 (G, k0, Nc), d0 (G, Nc)
    on the host or None.  -> (pick, pivot, LT, d) on the host."""
    from vargp_amd import ops
    dev = lambda t: None if t is None else t.to(DEV)
    out = ops.greedy_select(theta.to(DEV), x.to(DEV), None if cand is None else cand.to(DEV, torch.int32), dev(LT0), dev(d0),
                            M=M, nu2=nu2, eps=eps, n_sets=G)
    pick, pivot, LT, d = [t.cpu() for t in out]
    Nc = x.shape[0] if cand is None else cand.shape[1]
    k0 = 0 if LT0 is None else LT0.shape[1]
    assert pick.shape == (G, M) and pick.dtype == torch.int32 and pivot.shape == (G, M) and pivot.dtype == torch.float32
    assert LT.shape == (G, k0 + M, Nc) and d.shape == (G, Nc) and LT.dtype == d.dtype == torch.float32
    g2 = math.exp(2.0 * theta[-1].item())
    worst = [0.0, 0.0, 0.0, 0.0]          # pivot, row, d as fractions of their bounds; the largest err32
    for g in range(G):
        pk = pick[g].long()
        assert bool(((pk >= 0) & (pk < Nc)).all()) and pk.unique().numel() == M, f'{tag} set {g}: picks {pk.tolist()}'
        args = (x, None if cand is None else cand[g], theta, nu2, M, eps)
        kw = dict(LT0=None if LT0 is None else LT0[g], d0=None if d0 is None else d0[g], picks=pk)
        _, pv64, LT64, d64, db64 = ref_greedy(*args, **kw)
        _, _, _, d32, db32 = _one_thread(lambda: ref_greedy(*args, dtype=torch.float32, **kw))
        err32 = max((db32.double() - db64).abs().max().item(), (d32.double() - d64).abs().max().item()) / g2
        e = (RTOL_SCALAR + 2.0 * err32) * g2
        worst[3] = max(worst[3], err32)
        selected = torch.zeros(Nc, dtype=torch.bool)
        for k in range(M):
            p, r = int(pk[k]), k0 + k
            key = db64[k].clone()
            key[selected] = -1.0
            top = key.max().item()
            if top >= eps + 2.0 * e:
                assert db64[k, p].item() >= top - 2.0 * e, f'{tag} set {g} step {k}: picked d {db64[k, p].item()} of max {top}'
            elif top <= eps - 2.0 * e:
                assert p == int((~selected).nonzero()[0]) and float(LT[g, r].abs().max()) == 0.0, f'{tag} set {g} step {k}'
            ep = abs(pivot[g, k].item() - pv64[k].item())
            assert ep <= e, f'{tag} set {g} step {k}: pivot {pivot[g, k].item()} vs {pv64[k].item()} (bound {e:.2e})'
            worst[0] = max(worst[0], ep / e)
            if pv64[k].item() > eps:
                er, br = (LT[g, r].double() - LT64[r]).abs().max().item(), e / math.sqrt(pv64[k].item())
                assert er <= br, f'{tag} set {g} step {k}: row err {er:.2e} (bound {br:.2e})'
                worst[1] = max(worst[1], er / br)
            else:
                assert float(LT[g, r].abs().max()) == 0.0, f'{tag} set {g} step {k}: exhausted, row not zero'
            selected[p] = True
        ed = (d[g].double() - d64).abs().max().item()
        assert ed <= e, f'{tag} set {g}: d err {ed:.2e} (bound {e:.2e})'
        worst[2] = max(worst[2], ed / e)
        if k0:
            assert torch.equal(LT[g, :k0], LT0[g])
    print(f'{tag}: pivot {worst[0]:.3f} row {worst[1]:.3f} d {worst[2]:.3f} of the bound; fp32 host err32 {worst[3]:.1e}')
    return pick, pivot, LT, d


def _cases():
    """(tag, D, N, Nc or None = all rows in order, M, k0) -- the kernel code and the number of sets cycle over the list."""
    cases = [(f'D{D}', D, 257, None, 24, 0) for D in (1, 2, 32, 33, 40, 784)]
    for Nc in (1, 63, 65, 130):
        for M in sorted({1, min(5, Nc), Nc}):
            cases.append((f'Nc{Nc}-M{M}', 7, Nc, None, M, 0))
    cases += [('k0=3', 5, 200, 130, 10, 3), ('k0=37', 40, 200, 130, 10, 37), ('subset', 12, 400, 130, 9, 0)]
    return [c + ((0, 1, 3, 5)[i % 4], (1, 3)[(i // 4 + i) % 2]) for i, c in enumerate(cases)]


@pytest.mark.parametrize('tag,D,N,Nc,M,k0,nu2,G', _cases(), ids=[c[0] for c in _cases()])
def test_select_against_fp64(tag, D, N, Nc, M, k0, nu2, G):
    from vargp_amd import init
    x = clustered(N, D, seed=20 + D + N)
    theta = median_theta(x) if N > 1 else torch.tensor([0.0] * D + [math.log(0.5)])
    gen = torch.Generator().manual_seed(3)
    cand = None if Nc is None else torch.stack([torch.randperm(N, generator=gen)[:Nc] for _ in range(G)])
    LT0 = d0 = None
    if k0:
        # the prefill of init.greedy_inducing from random points, itself held to fp64 by the rule (entries of A against its
        # largest, d0 against gamma^2)
        z_prev = 2.0 * torch.randn(G, k0, D, generator=gen)
        pre = [init.whitened_cross(theta.to(DEV), z_prev[g].to(DEV), x[cand[g]].to(DEV), nu2) for g in range(G)]
        LT0, d0 = torch.stack([p[0] for p in pre]).cpu(), torch.stack([p[1] for p in pre]).cpu()
        g2 = math.exp(2.0 * theta[-1].item())
        for g in range(G):
            A64, dd64 = ref_whitened_cross(theta, z_prev[g], x[cand[g]], nu2, JITTER)
            A32, dd32 = _one_thread(lambda: ref_whitened_cross(theta, z_prev[g], x[cand[g]], nu2, JITTER, dtype=torch.float32))
            sa = A64.abs().max().item()
            ea, ea32 = (LT0[g].double() - A64).abs().max().item() / sa, (A32.double() - A64).abs().max().item() / sa
            ed, ed32 = (d0[g].double() - dd64).abs().max().item() / g2, (dd32.double() - dd64).abs().max().item() / g2
            print(f'{tag} set {g} prefill: A err {ea:.2e} (fp32 host {ea32:.2e}), d0 err {ed:.2e} (fp32 host {ed32:.2e})')
            assert ea <= RTOL_SCALAR + 2.0 * ea32 and ed <= RTOL_SCALAR + 2.0 * ed32
    _check(x, cand, theta, nu2, M, G, tag, LT0=LT0, d0=d0)


def test_argmax_across_workgroups_and_the_ragged_tile():
    """Three tiles of 64 candidates and a ragged fourth per set: one tight cluster and a far outlier at the LAST position.  Step 0
    picks position 0 (all keys tie), step 1 must find the outlier from another workgroup's tile."""
    Nc, D = 3 * 64 + 9, 6
    gen = torch.Generator().manual_seed(8)
    x = 0.01 * torch.randn(Nc, D, generator=gen)
    x[-1] += 5.0
    theta = torch.tensor([0.0] * D + [0.0])
    pick, pivot, _, _ = _check(x, None, theta, 0, 3, 2, 'outlier')
    assert pick[:, 0].tolist() == [0, 0] and pick[:, 1].tolist() == [Nc - 1, Nc - 1]
    assert bool((pivot[:, 1] > 0.999).all())


def test_duplicates_are_never_picked_twice():
    """Every point twice (Nc = 2 x 40, M = 30, D = 3): after a pick its twin has no variance left, so no pick is the twin of an
    earlier one."""
    gen = torch.Generator().manual_seed(9)
    base = torch.randn(40, 3, generator=gen)
    x = torch.cat([base, base])[torch.randperm(80, generator=gen)]
    theta = torch.tensor([math.log(0.3)] * 3 + [0.0])
    pick, pivot, _, _ = _check(x, None, theta, 5, 30, 1, 'twins')
    rows = x[pick[0].long()]
    assert torch.unique(rows, dim=0).shape[0] == 30
    assert bool((pivot > JITTER).all())


def test_exhaustion():
    """5 distinct points repeated to Nc = 20, M = 8: five picks of distinct points, then pivots <= eps, the lowest unselected
    positions and rows of zeros."""
    base = clustered(5, 4, seed=2)
    x = base.repeat(4, 1)
    theta = torch.tensor([0.0] * 4 + [0.0])
    pick, pivot, LT, _ = _check(x, None, theta, 3, 8, 3, 'exhaustion')
    for g in range(3):
        first = pick[g, :5].tolist()
        assert sorted(p % 5 for p in first) == [0, 1, 2, 3, 4]
        assert bool((pivot[g, 5:] <= JITTER).all()) and bool((pivot[g, :5] > JITTER).all())
        assert pick[g, 5:].tolist() == [i for i in range(20) if i not in first][:3]
        assert float(LT[g, 5:].abs().max()) == 0.0


def test_two_calls_are_bitwise_equal():
    from vargp_amd import ops
    x = clustered(300, 40, seed=4)
    theta = median_theta(x).to(DEV)
    gen = torch.Generator().manual_seed(1)
    cand = torch.stack([torch.randperm(300, generator=gen)[:257] for _ in range(3)]).to(DEV, torch.int32)
    a = ops.greedy_select(theta, x.to(DEV), cand, M=20, nu2=3)
    junk = torch.full((1 << 20,), float('nan'), device=DEV)            # (the pooled scratch is reused: poison what follows it)
    b = ops.greedy_select(theta, x.to(DEV), cand, M=20, nu2=3)
    del junk
    assert all(torch.equal(u, v) for u, v in zip(a, b))


# -- init ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D,nu2', [(5, 0), (5, 3), (784, 0), (784, 3)])
def test_greedy_inducing_rows_and_residual(D, nu2):
    """Rows of x bit for bit; the residual they leave (init.nystrom_residual, itself compared with its fp64 restatement) is below
    the mean over 20 random subsets; started from z_prev, [z_prev, z_greedy] leaves at most what [z_prev, z_random] leaves on
    average."""
    from vargp_amd import init
    N, M, C = 257, 24, 2
    x = clustered(N, D, seed=11)
    theta = median_theta(x)
    xd, thd = x.to(DEV), theta.to(DEV)
    torch.manual_seed(6)
    z = init.greedy_inducing(xd, C, M, thd, nu2=nu2)
    assert torch.equal(torch.get_rng_state(), _state_after(6, N, C))           # one randperm(N) per output, nothing else
    torch.manual_seed(6)
    cand = init.draw_candidates(N, C, 4096)
    assert z.shape == (C, M, D) and z.dtype == torch.float32
    zc = z.cpu()
    for g in range(C):
        same = (zc[g][:, None, :] == x[None, :, :]).all(-1)                     # (M, N)
        assert bool(same.any(-1).all()) and torch.equal(zc[g, 0], x[cand[g, 0]])
    res = init.nystrom_residual(xd, z, thd, nu2=nu2).cpu()
    assert res.shape == (C,) and res.dtype == torch.float64
    rand = random_subsets_residual(x, theta, nu2, M)
    mean_rand = sum(rand) / len(rand)
    for g in range(C):
        r64 = ref_residual(x, zc[g], theta, nu2)
        r32 = _one_thread(lambda: ref_residual(x, zc[g], theta, nu2, dtype=torch.float32))
        print(f'D={D} nu2={nu2} set {g}: greedy {res[g].item():.6g} (fp64 {r64:.6g}, fp32 host {r32:.6g}), random mean {mean_rand:.4g}')
        assert abs(res[g].item() - r64) <= RTOL_SCALAR * 0.25 + 2.0 * abs(r32 - r64)           # the rule, in units of gamma^2 = 0.25
        assert res[g].item() < mean_rand
    # started from the inducing points of an earlier task: 8 points of the first two clusters' side of the data
    z_prev = x[torch.randperm(N, generator=torch.Generator().manual_seed(2))[:8]]
    zp = z_prev.to(DEV).unsqueeze(0).expand(C, -1, -1).contiguous()
    zg = init.greedy_inducing(xd, C, M, thd, nu2=nu2, z_prev=zp)
    both = init.nystrom_residual(xd, torch.cat([zp, zg], 1), thd, nu2=nu2).cpu()
    rand_prev = random_subsets_residual(x, theta, nu2, M, z_prev=z_prev)
    print(f'D={D} nu2={nu2} with z_prev: greedy {both.tolist()}, random mean {sum(rand_prev) / len(rand_prev):.4g}')
    assert bool((both <= sum(rand_prev) / len(rand_prev)).all())
    with pytest.raises(ValueError):
        init.greedy_inducing(xd, C, N + 1, thd)
    with pytest.raises(ValueError):
        init.greedy_inducing(xd, C, 9, thd, n_candidates=8)


def _state_after(seed, N, n_draws):
    """the global CPU generator's state after n_draws randperm(N) from manual_seed(seed); the generator is left in that state."""
    torch.manual_seed(seed)
    for _ in range(n_draws):
        torch.randperm(N)
    return torch.get_rng_state()


# -- the factories ------------------------------------------------------------------------------------------------------------------
class _Data:
    def __init__(self, x, targets):
        self.x, self.targets = x, targets

    def __len__(self):
        return self.x.shape[0]

    def __getitem__(self, i):
        return self.x[i], self.targets[i]


@pytest.mark.parametrize('which', ['clf', 'reg'])
@pytest.mark.parametrize('kernel,median', [('rbf', False), ('rbf', True), ('matern32', False)])
def test_factories_greedy(which, kernel, median):
    """z_init='greedy' on a first task and with one previous task: z (C, M, D) of rows of the dataset, one finite loss().backward(),
    and the global CPU generator advanced by exactly out_size randperm draws where the random route draws (what follows them --
    the kernel's own draws, the median's pairs -- is then the random route's too: log_mean is compared)."""
    from vargp_amd.vargp import VARGP
    N, D, M = 300, 40, 6
    gen = torch.Generator().manual_seed(12)
    blob = torch.arange(N) % 6
    x = (3.0 * torch.randn(6, D, generator=gen))[blob] + 0.3 * torch.randn(N, D, generator=gen)
    if which == 'clf':
        data, make, C, y = _Data(x, blob), VARGP.create_clf, 6, blob[:64]
    else:
        t = torch.stack([x[:, 0] + 0.1 * torch.randn(N, generator=gen), x[:, 1] - x[:, 2]], -1)
        data, make, C, y = _Data(x, t), VARGP.create_reg, 2, t[:64].t().contiguous()
    kw = dict(M=M, kernel=kernel, lengthscale_init='median' if median else 'default')
    prev = None
    for task in range(2):
        torch.manual_seed(task)
        ref = make(data, prev_params=None if prev is None else [dict(p) for p in prev], **kw)
        after_ref = torch.get_rng_state()
        torch.manual_seed(task)
        gp = make(data, prev_params=None if prev is None else [dict(p) for p in prev], z_init='greedy', greedy_candidates=128, **kw)
        assert torch.equal(torch.get_rng_state(), after_ref)                  # the same draws, in number and kind
        assert torch.equal(gp.kernel.log_mean.detach(), ref.kernel.log_mean.detach())
        assert gp.z.shape == ref.z.shape == (C, M, D) and gp.z.dtype == ref.z.dtype and gp.z.device == ref.z.device
        torch.manual_seed(task)
        cand = torch.stack([torch.randperm(N)[:128] for _ in range(C)])
        z = gp.z.detach()
        for c in range(C):
            same = (z[c][:, None, :] == x[cand[c]][None, :, :]).all(-1)       # rows of the dataset, among ITS candidates
            assert bool(same.any(-1).all())
            assert torch.unique(z[c], dim=0).shape[0] == M
        if task == 0:
            assert torch.equal(z[:, 0], torch.stack([x[cand[c, 0]] for c in range(C)]))      # an empty start: the first candidate
        gp = gp.to(DEV)
        kl_h, kl_u, nll = gp.loss(x[:64].to(DEV), y.to(DEV))
        (kl_h + kl_u + nll).backward()
        for v in (kl_h, kl_u, nll):
            assert torch.isfinite(v).all()
        for name, p in gp.named_parameters():
            if p.grad is not None:
                assert torch.isfinite(p.grad).all(), name
        prev = [{k: v.detach().cpu().clone() for k, v in gp.state_dict().items()}]
