"""RBF / ARD kernel with a variational Normal over log-hyperparameters.

API of the reference's `var_gp.kernels.RBFKernel` (var_gp/kernels.py:7-77); the kernel matrices are
built by `vargp_rbf_gram_{fwd,bwd}` (f32-MFMA distance GEMM with fused exp epilogue).
"""
import math

import torch
import torch.nn as nn

from . import noise, ops


class RBFKernel(nn.Module):
    def __init__(self, in_size, prior_log_mean=None, prior_log_logvar=None, map_est=False):
        super().__init__()
        self.map_est = map_est
        # variational parameters over theta = [log lengthscale_1..D, log gamma]  (kernels.py:14-17)
        self.log_mean = nn.Parameter(math.log(0.5) + 0.05 * torch.randn(in_size + 1))
        self.log_logvar = nn.Parameter(torch.full((in_size + 1,), -2.0))
        # hyper-prior (kernels.py:19-22)
        self.register_buffer('prior_log_mean', torch.zeros(in_size + 1) if prior_log_mean is None
                             else prior_log_mean.detach().clone())
        self.register_buffer('prior_log_logvar', torch.zeros(in_size + 1) if prior_log_logvar is None
                             else prior_log_logvar.detach().clone())

    def set_lengthscale_(self, ell):
        """Start every lengthscale at ell > 0 (not in the reference: init.median_lengthscale supplies a data-dependent one):
        log_mean[:D] = log(ell) in place; the log gamma entry and log_logvar stay as they are.  For DeepRBFKernel these are
        the lengthscales of the feature space."""
        if not ell > 0:
            raise ValueError(f'set_lengthscale_: the lengthscale must be positive, got {ell!r}')
        with torch.no_grad():
            self.log_mean[:-1] = math.log(ell)
        return self

    def compute(self, kern_samples, x, y=None):
        """kern_samples (S, D+1); x (...batch, M, D); y (...batch, N, D) or None (= x).
        Returns (S, ...batch, M, N)  (kernels.py:24-56).  A `y` that is an expand() of one (N, D)
        block over the batch dims (how the reference feeds the minibatch, vargp.py:106) is consumed
        without materialising the copies."""
        return self._compute(ops.rbf_gram, kern_samples, x, y)

    @staticmethod
    def _compute(gram, kern_samples, x, y):
        """compute() around one of the gram ops (theta, X (C, M, D), Y, y_shared) -> (S, C, M, N)."""
        batch = x.shape[:-2]
        M, D = x.shape[-2:]
        X = x.reshape(-1, M, D)
        Y, shared = None, False
        if y is not None:
            N = y.shape[-2]
            if y.dim() == 2 or all(st == 0 or sz == 1 for st, sz in zip(y.stride()[:-2], y.shape[:-2])):
                Y, shared = y[(0,) * (y.dim() - 2)], True
            else:
                Y = y.expand(*batch, N, D).reshape(-1, N, D)
        K = gram(kern_samples, X, Y, shared)
        return K.reshape(kern_samples.shape[0], *batch, M, K.shape[-1])

    def compute_cov(self, kern_samples, x, P, W):
        """Full predictive covariance of the block x (B, D): K(x, x) - P^T P + W^T W, (S, C, B, B), in one fused pass
        (ops.predictive_cov; P, W (S, C, Mt, B) from gp_utils.marginal_apply_full).  No autograd."""
        return ops.predictive_cov(kern_samples, x, P, W, nu2=0)

    def compute_diag(self, kern_samples):
        """gamma^2 as (S, 1, 1)  (kernels.py:58-60)."""
        return (2.0 * kern_samples[..., -1:]).exp().unsqueeze(-2)

    def spectral_frequencies(self, n_features, device):
        """omega (R, D), R = n_features draws from the spectral law of the kernel at unit lengthscales -- N(0, I) for
        exp(-d2 / 2) -- so that gamma^2 / R sum_r cos((x - y) / lengthscale . omega_r) -> k(x, y) (paths.py; not in the
        reference).  Pure torch, any device; the noise is noise.draw('rff_omega', (R, D))."""
        return noise.draw('rff_omega', (int(n_features), self.log_mean.shape[0] - 1), device)

    def sample_hypers(self, n_hypers):
        """reparameterised theta ~ N(log_mean, exp(log_logvar))  (kernels.py:62-68)."""
        if self.map_est:
            return self.log_mean.unsqueeze(0)
        eps = noise.draw('eps_theta', (n_hypers, self.log_mean.shape[0]), self.log_mean.device)
        return ops.hyper_sample(self.log_mean, self.log_logvar, eps)

    def kl_hypers(self):
        """sum_d KL(q(theta_d) || p(theta_d)), both diagonal Normals  (kernels.py:70-77)."""
        if self.map_est:
            return torch.tensor(0.0, device=self.log_mean.device)
        return ops.hyper_kl(self.log_mean, self.log_logvar, self.prior_log_mean, self.prior_log_logvar)


class MaternKernel(RBFKernel):
    """Matern kernel, nu in {1/2, 3/2, 5/2}, on the RBF's scaled distance r = |(x - y) / lengthscale|:
    gamma^2 exp(-r), gamma^2 (1 + sqrt3 r) exp(-sqrt3 r), gamma^2 (1 + sqrt5 r + 5 r^2 / 3) exp(-sqrt5 r).
    Same hyper-parameters, priors and state dict as RBFKernel (`nu` and `native` are constructor arguments, not state);
    `compute` builds the kernel matrices with `vargp_matern_gram_{fwd,bwd}`.  native=False (the default): a model with this
    kernel runs the composed per-op route.  native=True: it runs the block ELBO program (csrc/elbo_tn.hip with the Matern
    epilogues, `native_code`), like an RBFKernel model on that program."""

    def __init__(self, in_size, nu=2.5, prior_log_mean=None, prior_log_logvar=None, map_est=False, native=False):
        if nu not in (0.5, 1.5, 2.5):
            raise ValueError(f'MaternKernel: nu must be 0.5, 1.5 or 2.5, got {nu!r}')
        super().__init__(in_size, prior_log_mean=prior_log_mean, prior_log_logvar=prior_log_logvar, map_est=map_est)
        self.nu = float(nu)
        self.native = bool(native)

    def compute(self, kern_samples, x, y=None):
        nu = self.nu
        return self._compute(lambda th, X, Y, shared: ops.matern_gram(th, X, Y, shared, nu), kern_samples, x, y)

    def compute_cov(self, kern_samples, x, P, W):
        # (one op for native=False and native=True alike)
        return ops.predictive_cov(kern_samples, x, P, W, nu2=int(round(2 * self.nu)))

    def spectral_frequencies(self, n_features, device):
        """The Matern kernel is a scale mixture of RBF kernels, so its spectral law is multivariate t with nu2 = 2 nu degrees
        of freedom: omega_r = g_r sqrt(nu2 / chi2_r), g as for the RBF kernel and chi2_r the sum of the squares of the nu2
        standard normals noise.draw('rff_mix', (R, nu2))[r]."""
        nu2 = int(round(2 * self.nu))
        g = super().spectral_frequencies(n_features, device)
        chi2 = noise.draw('rff_mix', (int(n_features), nu2), device).square().sum(-1, keepdim=True)
        return g * (nu2 / chi2).sqrt()


def native_code(kernel):
    """Which kernel epilogue of the native ELBO programs a model with `kernel` runs on (vargp_elbo_tn_desc.kernel_nu2):
    0 for exactly RBFKernel, 1 | 3 | 5 (= 2 nu) for exactly MaternKernel built with native=True, None for anything else
    (DeepRBFKernel, subclasses, native=False): the composed per-op route.  The one place that decides the route."""
    if type(kernel) is RBFKernel:
        return 0
    if type(kernel) is MaternKernel and kernel.native:
        return int(round(2 * kernel.nu))
    return None


class DeepRBFKernel(RBFKernel):
    """RBF kernel on learned features phi(x) (reference: var_gp/kernels.py:80-96, the `dkl` ablation of
    VARGP.create_clf).  `phi` is the reference's nn.Sequential (same parameter names, so state dicts and the
    `kernel.phi.*` carry-over of create_clf are interchangeable); it is evaluated by ops.linear_act, i.e. the MFMA GEMM
    with a fused bias / ReLU pass, forward and backward."""

    def __init__(self, in_size, feature_size=64, **kwargs):
        super().__init__(feature_size, **kwargs)
        self.phi = nn.Sequential(
            nn.Linear(in_size, 256),
            nn.ReLU(),
            nn.Linear(256, 256),
            nn.ReLU(),
            nn.Linear(256, feature_size),
        )

    def features(self, x):
        h = ops.linear_act(x, self.phi[0].weight, self.phi[0].bias, True)
        h = ops.linear_act(h, self.phi[2].weight, self.phi[2].bias, True)
        return ops.linear_act(h, self.phi[4].weight, self.phi[4].bias, False)

    def compute(self, kern_samples, x, y=None):
        x = self.features(x)
        if y is not None:
            if y.dim() > 2 and all(st == 0 or sz == 1 for st, sz in zip(y.stride()[:-2], y.shape[:-2])):
                y = y[(0,) * (y.dim() - 2)]           # an expand() of one (N, D) block: map it once
            y = self.features(y)
        return super().compute(kern_samples, x, y=y)

    def compute_cov(self, kern_samples, x, P, W):
        return super().compute_cov(kern_samples, self.features(x), P, W)
