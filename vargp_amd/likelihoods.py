"""Likelihoods of the reference's `var_gp.likelihoods` (same names, constructors and methods):
  * MulticlassSoftmax (var_gp/likelihoods.py:7-63): Monte-Carlo softmax on the fused `vargp_softmax_*` kernels;
  * GaussianLikelihood (var_gp/likelihoods.py:66-110): independent multi-output Gaussian, closed form on the
    `vargp_gauss_nll_*` kernels (csrc/gauss_lik.hip); draws no noise."""
import torch
import torch.nn as nn

from . import noise, ops


class MulticlassSoftmax(nn.Module):
    def __init__(self, n_f=1):
        super().__init__()
        self.n_f = n_f

    def _eps(self, mu):
        S, C, B = mu.shape
        return noise.draw('eps_f', (S, self.n_f, C, B), mu.device)

    def forward(self, mu, var):
        """log-softmax over classes of f = mu + sqrt(var) eps, (S, F, C, B)  (likelihoods.py:13-31).
        Not on the hot path (loss/predict use the fused kernels); kept for API compatibility."""
        f = mu.unsqueeze(1) + var.sqrt().unsqueeze(1) * self._eps(mu)
        return torch.log_softmax(f, dim=-2)

    def loss(self, pred_mu, pred_var, y):
        """sum_b mean_{s,f} -log p(y_b | f_sfb)  (likelihoods.py:33-47)."""
        return ops.softmax_nll(pred_mu, pred_var, self._eps(pred_mu), y)

    def predict(self, mu, var):
        """class probabilities (B, C) averaged over the S*F samples  (likelihoods.py:49-63)."""
        return ops.softmax_predict(mu, var, self._eps(mu))


class GaussianLikelihood(nn.Module):
    """Independent multi-output Gaussian likelihood with one learned observation log-variance per output."""

    def __init__(self, out_size, init_log_var=-4.):
        super().__init__()
        self.obs_log_var = nn.Parameter(init_log_var * torch.ones(out_size))

    def forward(self, mu, var):
        """observation mean and variance (S, C, B, 1) each  (likelihoods.py:74-89).  Not on the hot path; kept for API
        compatibility."""
        return mu.unsqueeze(-1), var.unsqueeze(-1) + self.obs_log_var.exp().view(1, -1, 1, 1)

    def loss(self, pred_mu, pred_var, y):
        """sum_b mean_{s,c} -log N(y | mu, var + exp(obs_log_var))  (likelihoods.py:91-107); y (C, B) or (B,)."""
        return ops.gauss_nll(pred_mu, pred_var, y, self.obs_log_var)

    def predict(self, mu, var):
        """the predictive mean itself, (S, C, B)  (likelihoods.py:109-110)."""
        return mu


def n_f(likelihood):
    """Monte-Carlo likelihood samples per hyper-sample: the F of the native programs' shapes.  The Gaussian likelihood is
    evaluated in closed form (the programs run it with ext_lik and F = 1)."""
    return 1 if isinstance(likelihood, GaussianLikelihood) else likelihood.n_f


def is_gaussian(likelihood):
    return isinstance(likelihood, GaussianLikelihood)
