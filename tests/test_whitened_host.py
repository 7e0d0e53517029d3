"""vargp_amd/whitened.py on the host: the pieces that are plain fp64 torch (the KL term, the inverse softplus) and the model
checker behind the five public checkers of collapsed.py and sites.py, whose texts are the ones those checkers raised before they
shared it.  No device."""
from types import SimpleNamespace

import pytest
import torch

F64 = torch.float64


@pytest.mark.parametrize('M', [1, 5])
def test_kl_standard_is_the_kl_of_the_distributions(M):
    """kl_standard(a, H) against torch.distributions' KL(N(a, H H^T) || N(0, I)), both in fp64: 1e-12 relative."""
    from torch.distributions import MultivariateNormal, kl_divergence
    from vargp_amd.whitened import kl_standard
    g = torch.Generator().manual_seed(M)
    C = 3
    a = torch.randn(C, M, generator=g, dtype=F64)
    H = torch.randn(C, M, M, generator=g, dtype=F64).tril()
    H = H - H.diagonal(dim1=-2, dim2=-1).diag_embed() + (0.3 + torch.rand(C, M, generator=g, dtype=F64)).diag_embed()
    ref = kl_divergence(MultivariateNormal(a, scale_tril=H), MultivariateNormal(torch.zeros(C, M, dtype=F64), scale_tril=torch.eye(M, dtype=F64).expand(C, M, M)))
    got = kl_standard(a, H)
    assert got.dtype == F64 and tuple(got.shape) == (C,)
    print(f'M={M}: kl {got.tolist()} reference {ref.tolist()}')
    assert torch.allclose(got, ref, rtol=1e-12, atol=0.0)


def test_inv_softplus_round_trips_through_softplus():
    from vargp_amd.whitened import inv_softplus
    d = torch.tensor([1e-6, 1.0, 30.0], dtype=F64)
    assert torch.allclose(torch.nn.functional.softplus(inv_softplus(d)), d, rtol=1e-12, atol=0.0)


def _gp(lik, kernel, mask=1.0, C=2):
    return SimpleNamespace(likelihood=lik, kernel=kernel, var_mean_mask=mask, z=torch.zeros(C, 4, 3))


EP = ('W: supported for ep_var_mean=True models only (with ep_var_mean=False the mean of q(u_t) is not u_mean alone)')
KERNELS = 'W: supported kernels are RBFKernel, MaternKernel and DeepRBFKernel, got Identity'
EXACT = 'W: supported kernels are exactly RBFKernel and MaternKernel, got _Sub'
GAUSS_ONLY = ('W: the closed-form q(u) exists for GaussianLikelihood only (create_reg(likelihood="gaussian")), got '
              'BernoulliLikelihood')
COUPLES = ('W: MulticlassSoftmax couples the outputs of a point, so it has no independent Gaussian sites; its own fit is '
           'fit_q_softmax_ (create_clf(q_init="newton_softmax")), or use create_clf(likelihood="bernoulli") for a one-vs-rest '
           'classifier')
CLOSED = 'W: for GaussianLikelihood the optimal q(u) has a closed form, use fit_q_'
SITE_LIKS = 'W: supported likelihoods are BernoulliLikelihood, PoissonLikelihood and StudentTLikelihood, got Identity'
SOFTMAX_ONLY = ('W: supported for MulticlassSoftmax only, got BernoulliLikelihood; the likelihoods with independent outputs have '
                'fit_q_newton_ (q_init="newton"), GaussianLikelihood has fit_q_')
DEEP_MOMENTS = ('W: DeepRBFKernel is not supported (the feature map needs the gradient of the moments for their inputs X, which the '
                'fused backward does not produce); fit_q_ supports it')
DEEP_SITES = ('W: DeepRBFKernel is not supported (the feature map needs the gradient of the site pass for its inputs X, which the '
              'fused backward does not produce); fit_q_newton_ supports it')


def test_the_public_checkers_keep_their_texts():
    """Every message of collapsed.check_supported / check_differentiable and sites.check_supported / check_softmax_supported /
    check_differentiable, in full, and the order in which a model with several faults is refused."""
    from vargp_amd import collapsed, ops, sites
    from vargp_amd.kernels import DeepRBFKernel, MaternKernel, RBFKernel
    from vargp_amd.likelihoods import BernoulliLikelihood, GaussianLikelihood, MulticlassSoftmax, PoissonLikelihood

    class _Sub(RBFKernel):
        pass

    rbf, matern, deep, sub, other = RBFKernel(3), MaternKernel(3, nu=1.5), DeepRBFKernel(3, feature_size=6), _Sub(3), torch.nn.Identity()
    gauss, bern, pois, soft = GaussianLikelihood(2), BernoulliLikelihood(), PoissonLikelihood(), MulticlassSoftmax(n_f=2)

    def refused(check, gp, text):
        with pytest.raises(ValueError) as e:
            check(gp, 'W')
        assert str(e.value) == text, (str(e.value), text)

    for check, lik, wrong in ((collapsed.check_supported, gauss, GAUSS_ONLY), (collapsed.check_differentiable, gauss, GAUSS_ONLY),
                              (sites.check_supported, bern, COUPLES), (sites.check_differentiable, pois, COUPLES),
                              (sites.check_softmax_supported, soft, SOFTMAX_ONLY)):
        bad = soft if wrong is COUPLES else bern
        for k in (rbf, matern):
            check(_gp(lik, k), 'W')                                                   # a supported model passes
        refused(check, _gp(bad, rbf, mask=0.0), wrong)                                # the likelihood before ep_var_mean
        refused(check, _gp(lik, other, mask=0.0), EP)                                 # ep_var_mean before the kernel
        refused(check, _gp(lik, other), KERNELS)
    for check in (sites.check_supported, sites.check_differentiable):
        refused(check, _gp(gauss, rbf), CLOSED)
        refused(check, _gp(other, rbf), SITE_LIKS)
    for check, lik in ((collapsed.check_supported, gauss), (sites.check_supported, bern), (sites.check_softmax_supported, soft)):
        check(_gp(lik, deep), 'W')
        check(_gp(lik, sub), 'W')
    for check, lik, text in ((collapsed.check_differentiable, gauss, DEEP_MOMENTS), (sites.check_differentiable, bern, DEEP_SITES)):
        refused(check, _gp(soft, deep, mask=0.0), text)                               # the deep kernel before everything else
        refused(check, _gp(lik, sub), EXACT)
    refused(sites.check_softmax_supported, _gp(soft, rbf, C=ops.SOFTMAX_SITE_MAX_C + 1),
            f'W: at most {ops.SOFTMAX_SITE_MAX_C} classes, got {ops.SOFTMAX_SITE_MAX_C + 1}')
    assert collapsed.check_supported.__defaults__ == ('fit_q_',) and sites.check_supported.__defaults__ == ('fit_q_newton_',)
    assert sites.check_softmax_supported.__defaults__ == ('fit_q_softmax_',)
