"""Data-dependent initialisation (not in the reference, whose models start at M random data points per output and at
lengthscale 0.5 whatever the data is): k-means centres as inducing points -- Lloyd's algorithm on the device, ops.kmeans_assign
and ops.kmeans_update (csrc/kmeans.hip) -- and the median heuristic for the lengthscale.  Both are off by default and reached
through VARGP.create_clf / create_reg (z_init='kmeans', lengthscale_init='median')."""
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
