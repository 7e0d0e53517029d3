"""Likelihoods of the reference's `var_gp.likelihoods` (same names, constructors and methods):
  * MulticlassSoftmax (var_gp/likelihoods.py:7-63): Monte-Carlo softmax on the fused `vargp_softmax_*` kernels;
  * GaussianLikelihood (var_gp/likelihoods.py:66-110): independent multi-output Gaussian, closed form on the
    `vargp_gauss_nll_*` kernels (csrc/gauss_lik.hip); draws no noise;
and one that the reference does not have:
  * BernoulliLikelihood: independent outputs (binary, multi-label, one-vs-rest), a fixed 20-node Gauss-Hermite rule on the
    `vargp_bernoulli_*` kernels (csrc/bernoulli_lik.hip); deterministic, no parameters.
GaussianLikelihood and BernoulliLikelihood are "external": the native ELBO programs stop at the predictive moments and the KL
(ext_lik) and these classes complete the step through one protocol -- ext_param / ext_target / ext_value / ext_backward."""
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

    # -- the native programs' ext_lik route ------------------------------------------------------------------------------------
    def ext_param(self):
        """The likelihood's own differentiable tensor (at most one), or None."""
        return self.obs_log_var

    def ext_target(self, y, C, B):
        """y as the kernels read it, plus the detached parameter: what ext_value / ext_backward take."""
        return ops.gauss_target(y, C, B) + (self.obs_log_var.detach().contiguous(),)

    def ext_value(self, prog, target):
        """After a program forward with ext_lik: the nll of its moments into prog.scalars[2], completing the
        (kl_hypers, kl_u, nll) triple."""
        from .fused import lik_views
        mu, var, _, _ = lik_views(prog)
        yt, ldy, olv = target
        ops.gauss_nll_fwd(mu, var, yt, ldy, olv, prog.scalars[2:])

    def ext_backward(self, prog, target, seed, nll=None, grad=None):
        """Before the program's backward: ONE launch -- the seeded d nll / d (mu, var) into the program's likelihood buffers,
        d nll / d ext_param() into `grad` (None: a new tensor), with `nll` the value too.  -> the parameter's gradient."""
        from .fused import lik_views
        mu, var, gmu, gvar = lik_views(prog)
        yt, ldy, olv = target
        grad = torch.empty_like(olv) if grad is None else grad
        ops.gauss_nll_bwd(mu, var, yt, ldy, olv, seed, gmu, gvar, grad, nll=nll)
        return grad


class BernoulliLikelihood(nn.Module):
    """Independent-output Bernoulli likelihood, p(t | f) = Lambda((2 t - 1) f) per output with Lambda the standard normal cdf
    (link='probit', the default) or the logistic function (link='logit').  Not in the reference.  No parameters, no
    Monte-Carlo noise (no n_f): the expected log-likelihood under f ~ N(mu, var) is DEFINED as the 20-node Gauss-Hermite sum
        ell = sum_k w_k / sqrt(pi) log Lambda((2 t - 1) (mu + sqrt(2 var) x_k)),   x, w = hermgauss(20),
    and the gradients are the exact derivatives of that sum.
    Against a 200-node rule, for |mu| <= 8 and var <= 4 its relative error is <= 3e-4 (probit) and <= 3e-6 (logit);
    at var <= 25 it is 5e-3.
    Targets: int64 (B,) class indices read as one-vs-rest (t[c, b] = (y[b] == c); a label outside [0, C) gives no positive
    output), or float / bool 0 / 1 targets (C, B) (multi-label) or (B,) (shared by every output).
    The loss SUMS over outputs: kl_u sums over outputs, so the ELBO of C independent outputs sums their log-likelihoods.
    (GaussianLikelihood keeps the reference's mean over outputs because it has the reference to match; this class has nothing
    to match.)"""

    def __init__(self, link='probit'):
        super().__init__()
        self.link = link
        self._link = ops.bernoulli_link(link)

    def forward(self, mu, var):
        """P(t = 1) per element, (S, C, B).  Not on the hot path; kept for API symmetry."""
        S, C, B = mu.shape
        return ops.bernoulli_predict(mu.reshape(1, S * C, B), var.reshape(1, S * C, B), self.link).t().reshape(S, C, B)

    def loss(self, pred_mu, pred_var, y):
        """- sum_b sum_c mean_s ell[s, c, b]; y as ops.bernoulli_target takes it."""
        return ops.bernoulli_nll(pred_mu, pred_var, y, self.link)

    def predict(self, mu, var):
        """probs (B, C) = mean_s P(t = 1), laid out like the softmax's so that an argmax over the last dim picks the class.
        The outputs are independent: a row is NOT normalised over c.  Probit: Phi(mu / sqrt(1 + var)) in closed form; logit:
        the 20-node rule on the logistic function."""
        return ops.bernoulli_predict(mu, var, self.link)

    # -- the native programs' ext_lik route (see GaussianLikelihood) ------------------------------------------------------------
    def ext_param(self):
        return None

    def ext_target(self, y, C, B):
        return ops.bernoulli_target(y, C, B)

    def ext_value(self, prog, target):
        from .fused import lik_views
        mu, var, _, _ = lik_views(prog)
        ops.bernoulli_nll_fwd(mu, var, *target, self._link, prog.scalars[2:])

    def ext_backward(self, prog, target, seed, nll=None, grad=None):
        from .fused import lik_views
        mu, var, gmu, gvar = lik_views(prog)
        ops.bernoulli_nll_bwd(mu, var, *target, self._link, seed, gmu, gvar, nll=nll)
        return None


def n_f(likelihood):
    """Monte-Carlo likelihood samples per hyper-sample: the F of the native programs' shapes.  The Gaussian likelihood is
    evaluated in closed form and the Bernoulli likelihood by a fixed rule (the programs run them with ext_lik and F = 1)."""
    return 1 if is_external(likelihood) else likelihood.n_f


def is_external(likelihood):
    """Is the likelihood the caller's -- do the native programs run it with ext_lik (moments + KL only) and leave value and
    gradients to the likelihood's ext_value / ext_backward?"""
    return isinstance(likelihood, (GaussianLikelihood, BernoulliLikelihood))


def is_gaussian(likelihood):
    return isinstance(likelihood, GaussianLikelihood)
