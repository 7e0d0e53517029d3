"""Likelihoods of the reference's `var_gp.likelihoods` (same names, constructors and methods):
  * MulticlassSoftmax (var_gp/likelihoods.py:7-63): Monte-Carlo softmax on the fused `vargp_softmax_*` kernels;
  * GaussianLikelihood (var_gp/likelihoods.py:66-110): independent multi-output Gaussian, closed form on the
    `vargp_gauss_nll_*` kernels (csrc/gauss_lik.hip); draws no noise;
and three that the reference does not have:
  * BernoulliLikelihood: independent outputs (binary, multi-label, one-vs-rest), a fixed 20-node Gauss-Hermite rule on the
    `vargp_bernoulli_*` kernels (csrc/indep_lik.hip); deterministic, no parameters;
  * PoissonLikelihood: counts with a log link, closed form on the `vargp_poisson_*` kernels (csrc/indep_lik.hip); no parameters;
  * StudentTLikelihood: robust regression, fixed degrees of freedom and one learned log-scale per output, the same 20-node
    rule on the `vargp_studentt_*` kernels (csrc/indep_lik.hip).
All but the softmax are "external" (_ExternalLikelihood): the native ELBO programs stop at the predictive moments and the KL
(ext_lik) and these classes complete the step through one protocol -- ext_param / ext_target / ext_value / ext_backward.
Every class names the layout of what its `predict` returns in `predict_batch_dim`: the dim that runs over the data points
(0 for probabilities (B, C), -1 for per-sample values (S, C, B)) -- what a tiled prediction concatenates along.
Every class has `log_prob(mu, var, y, per_output=False)`: the held-out log predictive density per point (B,), log E_q[p(y)] -- the
mixture over the hyper-samples of the marginal likelihood of the point's targets (csrc/lpd.hip; not in the reference, no gradients).
The classification likelihoods (softmax, Bernoulli) have `uncertainty(mu, var, per_output=False)`: the predictive entropy per point
split into noise and lack of knowledge (Uncertainty; csrc/uncertainty.hip; not in the reference, no gradients); the regression
likelihoods raise ValueError."""
from collections import namedtuple

import torch
import torch.nn as nn

from . import noise, ops


Uncertainty = namedtuple('Uncertainty', 'probs total aleatoric epistemic total_out aleatoric_out epistemic_out', defaults=(None,) * 3)
Uncertainty.__doc__ = """Predictive entropy per point, in nats: probs (B, C), the predictive probabilities the entropies belong to;
total (B,) = H[E p(y | theta, f)]; aleatoric (B,) = E H[p(y | theta, f)], the noise every sample agrees on; epistemic (B,) =
max(total - aleatoric, 0), the mutual information of the label and the model's random variables.  The three *_out (C, B): the
per-output values of independent outputs, whose sums over the outputs the (B,) arrays are; None unless asked for."""


def cat_uncertainty(parts):
    """One Uncertainty from those of consecutive blocks of points: probs (B, C) and the (B,) entropies run over the points in
    dim 0, the per-output arrays (C, B) in dim 1."""
    return Uncertainty(*(None if f[0] is None else torch.cat(f, dim=0 if k < 4 else 1) for k, f in enumerate(zip(*parts))))


class MulticlassSoftmax(nn.Module):
    predict_batch_dim = 0

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

    def log_prob(self, mu, var, y, per_output=False):
        """Held-out log predictive density (B,): log of the label's mean probability over the S F samples,
        logsumexp_{s,f} log_softmax(mu + sqrt(var) eps)[y] - log(S F).  The classes share one normaliser: there are no
        per-output marginals (per_output=True: ValueError)."""
        if per_output:
            raise ValueError('MulticlassSoftmax.log_prob: the softmax has no per-output marginals (per_output=True)')
        return ops.softmax_lpd(mu, var, self._eps(mu), y)

    def uncertainty(self, mu, var, per_output=False):
        """Uncertainty(probs (B, C), total, aleatoric, epistemic (B,)) of the S F samples p_sf = softmax(mu + sqrt(var) eps), eps
        drawn as predict draws it: probs = mean_sf p_sf (predict's definition), total = the entropy of probs, aleatoric =
        mean_sf of the entropy of p_sf, epistemic = max(total - aleatoric, 0); nats, 0 <= epistemic <= total <= log C.  The
        classes share one normaliser: there are no per-output parts (per_output=True: ValueError).  No gradients."""
        if per_output:
            raise ValueError('MulticlassSoftmax.uncertainty: the softmax has no per-output parts (per_output=True)')
        return Uncertainty(*ops.softmax_uncertainty(mu, var, self._eps(mu)))


class _ExternalLikelihood(nn.Module):
    """A likelihood with independent outputs on the uniform `vargp_<kind>_*` entries (ops.lik_nll_fwd / lik_nll_bwd / lik_lpd).
    A subclass names its `kind`, its own differentiable tensor (ext_param(): at most one (C,), or None) and its host constants
    (_consts()); `_extra()` is what the entries take between target and outputs: the DETACHED parameter -- a view of the
    parameter's storage, so one taken when a graph is captured stays current -- and the constants."""
    kind = None

    def ext_param(self):
        """The likelihood's own differentiable tensor (at most one), or None."""
        return None

    def _consts(self):
        return ()

    def _extra(self):
        own = self.ext_param()
        return (() if own is None else (own.detach().contiguous(),)) + self._consts()

    def loss(self, pred_mu, pred_var, y):
        """The nll of the moments (S, C, B): minus the expected log-likelihood under f ~ N(mu, var), summed over the points and
        averaged over the hyper-samples; y as the kind's ops.*_target takes it.  Differentiable in mu, var and ext_param()."""
        return ops.lik_nll(self.kind, pred_mu, pred_var, y, self.ext_param(), *self._consts())

    def log_prob(self, mu, var, y, per_output=False):
        """Held-out log predictive density: lpd (B,) = logsumexp_s sum_c lp[s, c, b] - log S, the joint density of a point's
        targets under the mixture over hyper-samples (they share the hyper-sample), with lp the log marginal likelihood of one
        target under f ~ N(mu, var); per_output: (lpd, lpd_out (C, B)) with the per-output marginals.  Not in the reference.
        No gradients."""
        return ops.lik_lpd(self.kind, mu, var, y, self._extra(), per_output)

    def uncertainty(self, mu, var, per_output=False):
        """The split of the predictive entropy into noise and lack of knowledge: classification likelihoods only
        (BernoulliLikelihood overrides this).  The entropy of a predictive mixture of densities has no closed form."""
        raise ValueError(f'{type(self).__name__}.uncertainty: the predictive entropy split is defined for the classification '
                         'likelihoods (MulticlassSoftmax, BernoulliLikelihood) only')

    # -- the native programs' ext_lik route ------------------------------------------------------------------------------------
    def ext_target(self, y, C, B):
        """(y as the kernels read it, _extra()): what ext_value / ext_backward take."""
        return ops.lik_target(self.kind, y, C, B), self._extra()

    def ext_value(self, prog, target):
        """After a program forward with ext_lik: the nll of its moments into prog.scalars[2], completing the
        (kl_hypers, kl_u, nll) triple."""
        from .fused import lik_views
        mu, var, _, _ = lik_views(prog)
        ops.lik_nll_fwd(self.kind, mu, var, *target, prog.scalars[2:])

    def ext_backward(self, prog, target, seed, nll=None, grad=None):
        """Before the program's backward: ONE launch -- the seeded d nll / d (mu, var) into the program's likelihood buffers,
        d nll / d ext_param() into `grad` (None: a new tensor), with `nll` the value too.  -> the parameter's gradient."""
        from .fused import lik_views
        mu, var, gmu, gvar = lik_views(prog)
        if grad is None and self.ext_param() is not None:
            grad = torch.empty_like(target[1][0])
        ops.lik_nll_bwd(self.kind, mu, var, *target, seed, gmu, gvar, grad, nll=nll)
        return grad


class GaussianLikelihood(_ExternalLikelihood):
    """Independent multi-output Gaussian likelihood with one learned observation log-variance per output.
    loss: sum_b mean_{s,c} -log N(y | mu, var + exp(obs_log_var))  (likelihoods.py:91-107), the reference's MEAN over outputs;
    y (C, B) or (B,).  log_prob: lp = log N(y | mu, var + exp(obs_log_var)), closed form."""
    predict_batch_dim = -1
    kind = 'gauss'

    def __init__(self, out_size, init_log_var=-4.):
        super().__init__()
        self.obs_log_var = nn.Parameter(init_log_var * torch.ones(out_size))

    def forward(self, mu, var):
        """observation mean and variance (S, C, B, 1) each  (likelihoods.py:74-89).  Not on the hot path; kept for API
        compatibility."""
        return mu.unsqueeze(-1), var.unsqueeze(-1) + self.obs_log_var.exp().view(1, -1, 1, 1)

    def predict(self, mu, var):
        """the predictive mean itself, (S, C, B)  (likelihoods.py:109-110)."""
        return mu

    def ext_param(self):
        return self.obs_log_var


class BernoulliLikelihood(_ExternalLikelihood):
    """Independent-output Bernoulli likelihood, p(t | f) = Lambda((2 t - 1) f) per output with Lambda the standard normal cdf
    (link='probit', the default) or the logistic function (link='logit').  Not in the reference.  No parameters, no
    Monte-Carlo noise (no n_f): the expected log-likelihood under f ~ N(mu, var) is DEFINED as the 20-node Gauss-Hermite sum
        ell = sum_k w_k / sqrt(pi) log Lambda((2 t - 1) (mu + sqrt(2 var) x_k)),   x, w = hermgauss(20),
    and the gradients are the exact derivatives of that sum.
    Against a 200-node rule, for |mu| <= 8 and var <= 4 its relative error is <= 3e-4 (probit) and <= 3e-6 (logit);
    at var <= 25 it is 5e-3.
    Targets: int64 (B,) class indices read as one-vs-rest (t[c, b] = (y[b] == c); a label outside [0, C) gives no positive
    output), or float / bool 0 / 1 targets (C, B) (multi-label) or (B,) (shared by every output).
    The loss SUMS over outputs, - sum_b sum_c mean_s ell[s, c, b]: kl_u sums over outputs, so the ELBO of C independent outputs
    sums their log-likelihoods.  (GaussianLikelihood keeps the reference's mean over outputs because it has the reference to
    match; this class has nothing to match.)
    log_prob: per element log Phi(s mu / sqrt(1 + var)) (probit) or the 20-node rule on the logistic function (logit)."""
    predict_batch_dim = 0
    kind = 'bernoulli'

    def __init__(self, link='probit'):
        super().__init__()
        self.link = link
        self._link = ops.bernoulli_link(link)

    def forward(self, mu, var):
        """P(t = 1) per element, (S, C, B).  Not on the hot path; kept for API symmetry."""
        S, C, B = mu.shape
        return ops.bernoulli_predict(mu.reshape(1, S * C, B), var.reshape(1, S * C, B), self.link).t().reshape(S, C, B)

    def predict(self, mu, var):
        """probs (B, C) = mean_s P(t = 1), laid out like the softmax's so that an argmax over the last dim picks the class.
        The outputs are independent: a row is NOT normalised over c.  Probit: Phi(mu / sqrt(1 + var)) in closed form; logit:
        the 20-node rule on the logistic function."""
        return ops.bernoulli_predict(mu, var, self.link)

    def uncertainty(self, mu, var, per_output=False):
        """Uncertainty(probs (B, C), total, aleatoric, epistemic (B,)) in nats, per output on the class's 20-node rule with
        h(p) = -p log p - (1 - p) log(1 - p): p_out = mean_s sum_k w_k Lambda(f_k), total_out = h(p_out), aleatoric_out =
        mean_s sum_k w_k h(Lambda(f_k)), epistemic_out = max(total_out - aleatoric_out, 0); the (B,) values are the sums over
        the outputs (the one-vs-rest score, an upper bound on the joint quantity).  per_output=True: the three (C, B) arrays
        are filled in too.  probs uses the rule for the probit link as well (one rule on both sides of Jensen's
        inequality): it differs from predict's closed form by the rule's quadrature error, documented on the class.  No
        gradients."""
        return Uncertainty(*ops.bernoulli_uncertainty(mu, var, self.link, per_output=per_output))

    def _consts(self):
        return (self._link,)


class PoissonLikelihood(_ExternalLikelihood):
    """Independent-output Poisson likelihood with a log link, p(y | f) = Poisson(y; exp(f)): counts.  Not in the reference.  No
    parameters, no noise, no quadrature -- under f ~ N(mu, var) the expected log-likelihood is closed form, with m = mu + var / 2:
        ell = y mu - exp(m) - lgamma(y + 1)
    Targets: non-negative floats (or integers, cast) of shape (C, B), or (B,) shared by every output; not checked on the device.
    exp(m) overflows fp32 above m ~ 88.7: value and gradients are then inf, as the formula says -- nothing is clamped.
    The loss SUMS over outputs and takes the mean over hyper-samples, - sum_b sum_c mean_s ell[s, c, b], as BernoulliLikelihood
    does: the ELBO of C independent outputs, C times GaussianLikelihood's (the reference's) mean-over-outputs convention.
    log_prob: the marginal likelihood of a count is the 20-node Gauss-Hermite sum of Poisson(y; exp(f_k))."""
    predict_batch_dim = -1
    kind = 'poisson'

    def forward(self, mu, var):
        """the rate E exp(f) per element, (S, C, B)."""
        return ops.poisson_predict(mu, var)

    def predict(self, mu, var):
        """the predicted rate exp(mu + var / 2) per hyper-sample, (S, C, B) -- the layout of GaussianLikelihood.predict."""
        return ops.poisson_predict(mu, var)


class StudentTLikelihood(_ExternalLikelihood):
    """Independent-output Student-t likelihood, p(y | f) = t_df((y - f) / sigma_c) / sigma_c with sigma_c = exp(log_scale[c]):
    regression that a few outliers do not pull along.  Not in the reference.  One learned log-scale per output; the degrees of
    freedom `df` > 0 are a fixed constructor argument and NOT part of the state dict -- give them again when a checkpoint is
    reloaded (as MaternKernel.nu).  No noise: the expected log-likelihood under f ~ N(mu, var) is DEFINED as the 20-node
    Gauss-Hermite sum (BernoulliLikelihood's rule)
        ell = K_c - (df + 1) / 2 sum_k w_k / sqrt(pi) log1p((y - mu - sqrt(2 var) x_k)^2 / (df sigma_c^2)),
        K_c = lgamma((df + 1) / 2) - lgamma(df / 2) - log(df pi) / 2 - log_scale[c],
    and the gradients are the exact derivatives of that sum.  (As an approximation of the integral the rule is as good as twenty
    nodes resolve the density's width: with sqrt(var) ten times sigma_c single terms are up to 6 % away from a 200-node rule.)
    Targets (C, B), or (B,) shared by every output.
    The loss SUMS over outputs and takes the mean over hyper-samples, - sum_b sum_c mean_s ell[s, c, b], as BernoulliLikelihood
    does: the ELBO of C independent outputs, C times GaussianLikelihood's (the reference's) mean-over-outputs convention.
    log_prob: the marginal likelihood of a target is the 20-node Gauss-Hermite sum of the Student-t density."""
    predict_batch_dim = -1
    kind = 'studentt'

    def __init__(self, out_size, df=4.0, init_log_scale=-2.):
        super().__init__()
        self.df = float(df)
        ops.studentt_lognorm(self.df)           # (ValueError unless df > 0)
        self.log_scale = nn.Parameter(init_log_scale * torch.ones(out_size))

    def forward(self, mu, var):
        """location and squared scale of the observation model around f's moments, (S, C, B, 1) each: mu, and
        var + exp(2 log_scale).  Not on the hot path; kept for API symmetry with GaussianLikelihood."""
        return mu.unsqueeze(-1), var.unsqueeze(-1) + (2 * self.log_scale).exp().view(1, -1, 1, 1)

    def predict(self, mu, var):
        """the predictive location, the mean itself, (S, C, B) -- as GaussianLikelihood.predict."""
        return mu

    def ext_param(self):
        return self.log_scale

    def _consts(self):
        return self.df, ops.studentt_lognorm(self.df)


def n_f(likelihood):
    """Monte-Carlo likelihood samples per hyper-sample: the F of the native programs' shapes.  The external likelihoods are
    evaluated in closed form (Gaussian, Poisson) or by a fixed rule (Bernoulli, Student-t): the programs run them with ext_lik
    and F = 1."""
    return 1 if is_external(likelihood) else likelihood.n_f


def is_external(likelihood):
    """Is the likelihood the caller's -- do the native programs run it with ext_lik (moments + KL only) and leave value and
    gradients to the likelihood's ext_value / ext_backward?"""
    return isinstance(likelihood, _ExternalLikelihood)


def is_gaussian(likelihood):
    return isinstance(likelihood, GaussianLikelihood)


def predict_batch_dim(likelihood):
    """The dim of likelihood.predict(...) that runs over the data points: what a tiled prediction concatenates along."""
    return likelihood.predict_batch_dim
