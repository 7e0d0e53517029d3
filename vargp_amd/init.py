"""Data-dependent initialisation (not in the reference, whose models start at M random data points per output and at
lengthscale 0.5 whatever the data is): k-means centres as inducing points -- Lloyd's algorithm on the device, ops.kmeans_assign
and ops.kmeans_update (csrc/kmeans.hip) -- and the median heuristic for the lengthscale.  Both are off by default and reached
through VARGP.create_clf / create_reg (z_init='kmeans', lengthscale_init='median').  Greedy conditional-variance selection
(greedy_inducing, z_init='greedy'; ops.greedy_select, csrc/greedy.hip) picks data points with the model's own kernel and can start
from the inducing points of earlier tasks; nystrom_residual is the yardstick for any inducing set."""
import math

import torch

from . import ops


def lloyd(x, z0, n_iter):
    """Lloyd's algorithm for G independent sets of centres over one data matrix: x (N, D), z0 (G, K, D), both on the device.
    -> (z (G, K, D), label int32 (G, N), inertia (G,) float64, n_done).  label and inertia (the sum of the squared distances to
    the nearest centre) belong to the returned z.  Stops early when an iteration changes no label: one host sync per
    iteration.  A centre that loses all its points stays where it is.  n_iter=0 returns z0 itself."""
    z = z0
    label, d2 = ops.kmeans_assign(x, z)
    n_done = 0
    for _ in range(int(n_iter)):
        z, _ = ops.kmeans_update(x, label, z)
        new_label, d2 = ops.kmeans_assign(x, z)
        n_done += 1
        same = torch.equal(new_label, label)
        label = new_label
        if same:
            break
    return z, label, d2.sum(-1, dtype=torch.float64), n_done


def kmeans_inducing(x, n_sets, M, n_iter=20):
    """Inducing points (n_sets, M, D) for a model with n_sets outputs: per output, Lloyd's algorithm over x (N, D, on the device)
    from M random data points.  The seeds are the draws VARGP.create_clf makes for its random initialisation (the same calls on
    the torch global generator, in the same order), so n_iter=0 reproduces that initialisation exactly."""
    N = x.shape[0]
    seeds = torch.stack([x[torch.randperm(N)[:M].to(x.device)] for _ in range(n_sets)])
    return lloyd(x, seeds, n_iter)[0]


def _gram(theta, X, Y, nu2):
    """K (1, 1, M, N) of one point set X (M, D) against Y (N, D), or against itself (Y None), at ONE hyper vector theta (D+1,)."""
    th, Xb = theta.reshape(1, -1), X.unsqueeze(0)
    return ops.rbf_gram(th, Xb, Y, Y is not None) if nu2 == 0 else ops.matern_gram(th, Xb, Y, Y is not None, nu=nu2 / 2.0)


def whitened_cross(theta, z, y, nu2=0, eps=ops.JITTER):
    """T K(z, y) (Mz, Ny), T the inverse Cholesky factor of K(z, z) + eps I, and gamma^2 - its column sums of squares clamped at
    0 (Ny,): what is left of the prior variance at y after conditioning on z.  z (Mz, D), y (Ny, D), one hyper vector; composed
    from the gram, chol_inv and bgemm ops.  This is the state a pivoted Cholesky over y has after the points z."""
    T = ops.chol_inv(_gram(theta, z, None, nu2), eps)[1]
    A = ops.bgemm(T, _gram(theta, z, y, nu2), triA=ops.LOWER)[0, 0]
    g2 = (2.0 * theta.reshape(-1)[-1]).exp()
    return A, (g2 - (A * A).sum(0)).clamp_min(0.0)


def draw_candidates(N, n_sets, n_candidates):
    """The candidate rows of greedy_inducing, int64 (n_sets, min(N, n_candidates)) on the CPU: per output one
    torch.randperm(N) on the global CPU generator, in output order -- the very draws of the random initialisation."""
    return torch.stack([torch.randperm(N)[:min(N, int(n_candidates))] for _ in range(n_sets)])


def greedy_inducing(x, n_sets, M, theta, nu2=0, n_candidates=4096, z_prev=None, eps=ops.JITTER, cand=None):
    """Inducing points (n_sets, M, D) by greedy conditional-variance selection (a pivoted Cholesky of the kernel matrix, Burt et
    al., JMLR 2020): per output, M times, the candidate with the largest variance left after conditioning on everything picked
    so far, under the kernel k(.; theta, nu2) -- theta (D+1,) ONE hyper vector (log lengthscales, log gamma), nu2 0 = RBF,
    1 | 3 | 5 = Matern.  x (N, D) on the device.  The candidates of an output are min(N, n_candidates) rows of x from one
    torch.randperm(N) on the global CPU generator (draw_candidates; cand= hands over rows drawn earlier), and their order is the
    random start: the first pick of an empty start is the first candidate.  4096 is a default, not a tuned value: the work and
    the traffic are linear in it, and one set's candidates at D = 784 are 12.8 MB.  z_prev (n_sets, Mp, D), the previous tasks'
    inducing points concatenated, starts the factorisation from them, so the new points go where those leave variance.  eps: the
    jitter of the model's Cholesky; once no candidate has more variance than that left, the remaining points are the first
    unpicked candidates.  The returned rows are bitwise copies of rows of x.  ValueError when M exceeds the candidate count."""
    ops.require_device(x, theta, z_prev)
    N = x.shape[0]
    if cand is None:
        cand = draw_candidates(N, n_sets, n_candidates)
    Nc = cand.shape[1]
    if M > Nc:
        raise ValueError(f'greedy_inducing: M = {M} inducing points from {Nc} candidates')
    assert cand.shape[0] == n_sets, (cand.shape, n_sets)
    cand = cand.to(device=x.device, dtype=torch.int32)
    theta = theta.detach().to(device=x.device, dtype=torch.float32).reshape(-1)
    LT0 = d0 = None
    if z_prev is not None and z_prev.shape[1] > 0:
        pre = [whitened_cross(theta, z_prev[g].detach(), x[cand[g].long()], nu2, eps) for g in range(n_sets)]
        LT0, d0 = torch.stack([p[0] for p in pre]), torch.stack([p[1] for p in pre])
    pick = ops.greedy_select(theta, x, cand, LT0, d0, M=M, nu2=nu2, eps=eps)[0]
    return x[torch.gather(cand, 1, pick).long()]


def nystrom_residual(x, z, theta, nu2=0, eps=ops.JITTER):
    """(n_sets,) float64: per set g, the mean over the rows of x (N, D) of gamma^2 - |T K(z_g, x)|^2, T the inverse Cholesky
    factor of K(z_g, z_g) + eps I -- the prior variance the inducing points z (n_sets, M, D) leave unexplained (the trace of the
    Nystrom residual over N), unclamped.  One set at a time, composed from the gram, chol_inv and bgemm ops."""
    ops.require_device(x, z, theta)
    theta = theta.detach().to(device=x.device, dtype=torch.float32).reshape(-1)
    g2 = (2.0 * theta[-1]).double().exp()
    out = []
    for zg in z.detach():
        T = ops.chol_inv(_gram(theta, zg, None, nu2), eps)[1]
        A = ops.bgemm(T, _gram(theta, zg, x, nu2), triA=ops.LOWER)[0, 0]
        out.append(g2 - (A * A).sum(0, dtype=torch.float64).mean())
    return torch.stack(out)


def median_lengthscale(x, n_pairs=4096, scale=1.0):
    """The median heuristic: scale * sqrt(median |x_i - x_j|^2) over n_pairs random pairs i != j of the rows of x (N >= 2, any
    device; plain torch).  With this lengthscale in every dimension the median pair sits at scaled squared distance 1 / scale^2,
    i.e. at kernel value exp(-1 / (2 scale^2)) of the RBF's gamma^2."""
    N = x.shape[0]
    if N < 2:
        raise ValueError(f'median_lengthscale: needs at least two points, got {N}')
    i = torch.randint(N, (int(n_pairs),))
    j = (i + torch.randint(1, N, (int(n_pairs),))) % N
    xf = x.reshape(N, -1)
    d2 = (xf[i.to(x.device)].double() - xf[j.to(x.device)].double()).pow(2).sum(-1)
    return float(scale) * math.sqrt(d2.median().item())
