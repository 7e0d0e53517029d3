"""Pathwise (Matheron / decoupled) samples of the posterior over the latent functions: functions that can be evaluated at any
points, as often as asked, at a cost linear in the number of points (not in the reference, whose only function-space
quantity is the marginal of one minibatch).

For hyper-sample s and output c, with R frequencies omega (kernel.spectral_frequencies) and Phi_s(x) = gamma_s / sqrt(R)
[cos p | sin p], p = (x / lengthscale_s) omega^T, path n is

    g(x) = Phi_s(x) w[s, c, :, n]                                    the prior path, w ~ N(0, I_2R)
    r    = Lz^-1 m + G eps_u[s, c, :, n] - Lz^-1 g(z_c)              G = Lz^-1 chol(S_u + eps I), eps_u ~ N(0, I_Mt)
    V    = Lz^-T r
    f(x) = g(x) + K(x, z_c) V                                        the update through the inducing points of all tasks

with (m, S_u) the moments of q(u_<=t | theta) and Lz = chol(K(z, z) + eps I), the factors of VARGP.predict_f.  E f is
predict_f's mean for any R; Cov f tends to predict_f's covariance less JITTER A A^T (A = P^T Lz^-1) as R grows.  The feature
products g(z) and g(x) are ops.rff_paths (csrc/rff.hip): the features never reach memory.  PosteriorPaths.differentiable
evaluates the same functions on the autograd graph of x (ops.rff_paths_x: a fused HIP backward in the points), which is
what following one sampled function along its slope needs (PosteriorPaths.ascend).
"""
import copy

import torch

from . import gp_utils, noise, ops
from .gp_utils import rev_cholesky, vec2tril
from .ops import LOWER, UPPER


class PosteriorPaths:
    """n_paths function draws per (hyper-sample, output) of `model`'s posterior, frozen at construction: the object keeps
    detached copies of theta, omega, the weights, V and z and its own copy of the kernel, so training the model afterwards
    does not change the sampled functions.  Noise by name (noise.inject): eps_theta, rff_omega (and rff_mix for a Matern
    kernel), rff_w (S, C, 2R, n_paths), eps_up (S, C, Mt, n_paths)."""

    def __init__(self, model, n_paths=1, n_features=1024):
        N, R = int(n_paths), int(n_features)
        if N < 1 or R < 1:
            raise ValueError(f'PosteriorPaths: n_paths and n_features must be positive, got {n_paths!r}, {n_features!r}')
        with torch.no_grad():
            kern = model.kernel
            theta = kern.sample_hypers(model.n_v)
            if model.prev_params:
                _, _, m, S_u, z = model.compute_q(theta)
            else:
                m, z = model.u_mean, model.z
                S_u = rev_cholesky(vec2tril(model.u_tril_vec, model.M))
            prep = gp_utils.marginal_prepare(m, S_u, kern.compute(theta, z))
            S, (C, Mt), dev = theta.shape[0], z.shape[:2], z.device
            omega = kern.spectral_frequencies(R, dev)
            coef = noise.draw('rff_w', (S, C, 2 * R, N), dev)
            eps_u = noise.draw('eps_up', (S, C, Mt, N), dev)
            self.kernel = copy.deepcopy(kern).requires_grad_(False)
            self.theta, self.omega, self.coef, self.z = (t.detach().clone() for t in (theta, omega, coef, z))
            gz = ops.rff_paths(self.theta, self._features(self.z), self.omega, self.coef, x_shared=False)      # (S, C, Mt, N)
            Tz = prep['Tz']
            r = ops.matmul(prep['G'], eps_u, D=prep['Lz_m'], beta=1.0, triA=LOWER)
            r = ops.matmul(Tz, gz, D=r, alpha=-1.0, beta=1.0, triA=LOWER)
            self.V = ops.matmul(Tz.mT, r, triA=UPPER).detach().clone()                                         # (S, C, Mt, N)
        self.n_paths, self.n_features = N, R

    def _features(self, x):
        """The inputs of the RBF head: x itself, or a deep kernel's feature map of it."""
        return self.kernel.features(x) if hasattr(self.kernel, 'features') else x

    def __call__(self, x, tile=None):
        """The paths at x (B, D) -> (n_paths, S, C, B), the layout of VARGP.sample_f.  With `tile`, x is swept in blocks of
        `tile` points (memory per block: K(z, x_block) and the block's values); every call, whatever its blocks, evaluates
        the same functions."""
        B = x.size(0)
        tile = B if tile is None else max(int(tile), 1)
        with torch.no_grad():
            out = []
            for i in range(0, B, tile):
                xb = x[i:i + tile]
                g = ops.rff_paths(self.theta, self._features(xb), self.omega, self.coef, x_shared=True)        # (S, C, b, N)
                Kzx = self.kernel.compute(self.theta, self.z, xb)                                              # (S, C, Mt, b)
                out.append(ops.matmul(Kzx.mT, self.V, D=g, beta=1.0))
            return torch.cat(out, dim=-2).permute(3, 0, 1, 2).contiguous()

    def differentiable(self, x):
        """The paths at x (B, D) -> (n_paths, S, C, B): the values of paths(x), attached to the autograd graph of x, so that
        torch.autograd.grad(f[k, s, c].sum(), x) is the slope of ONE sampled function at all B points (row b of x enters
        column b of f only).  Only x is differentiated: theta, omega, the weights, V, z and the kernel copy are frozen and never
        receive a gradient.  No `tile` here: the graph keeps K(z, x), S C Mt B floats, until the backward has run, whatever
        the blocks -- sweep x in blocks yourself where that is too much.  The feature product's backward is one fused kernel
        (ops.rff_paths_x): the S B 2R features are not saved."""
        theta, z, V = self.theta.detach(), self.z.detach(), self.V.detach()
        g = ops.rff_paths_x(theta, self._features(x), self.omega, self.coef, True)                             # (S, C, B, N)
        Kzx = self.kernel.compute(theta, z, x)                                                                 # (S, C, Mt, B)
        return ops.matmul(Kzx.mT, V, D=g, beta=1.0).permute(3, 0, 1, 2).contiguous()

    def ascend(self, x0, index, n_steps=100, step_size=1e-2):
        """Plain gradient ascent of the single function f[index], index = (k, s, c): path k of hyper-sample s and output c.
        x0 (B, D) is a set of starting points, one independent ascent per row, n_steps steps x <- x + step_size df/dx.
        -> (x (B, D), f(x) (B,)), detached.  Each function costs its own backward pass: ascending several of them means one
        call (and one backward per step) each."""
        k, s, c = index
        x = x0.detach().clone()
        for _ in range(int(n_steps)):
            x.requires_grad_(True)
            grad, = torch.autograd.grad(self.differentiable(x)[k, s, c].sum(), x)
            x = x.detach() + step_size * grad
        return x, self(x)[k, s, c]
