"""The refusals of the site families' Python surface that need no device, each with its FULL text: fit_q_newton_, fit_q_softmax_,
site_bound, softmax_site_bound, fit_sites_, fit_softmax_sites_, loo, the four model checkers of sites.py, and create_clf /
create_reg for every q_init.  The two families (independent outputs, softmax) share one skeleton per entry; the texts, the `who`
prefix of every entry and the order in which two bad arguments are refused are behaviour, and this file pins them.  Models of
C = 3, M = 4, D = 3, N = 40, as test_softmax_sites_host.py builds them (and one of 129 classes for the class cap)."""
import re

import pytest
import torch

from test_collapsed import _Data

N, D, C, M = 40, 3, 3, 4

EP = '{who}: supported for ep_var_mean=True models only (with ep_var_mean=False the mean of q(u_t) is not u_mean alone)'
COUPLED = ('{who}: MulticlassSoftmax couples the outputs of a point, so it has no independent Gaussian sites; its own fit is '
           'fit_q_softmax_ (create_clf(q_init="newton_softmax")), or use create_clf(likelihood="bernoulli") for a one-vs-rest '
           'classifier')
GAUSS = '{who}: for GaussianLikelihood the optimal q(u) has a closed form, use fit_q_'
INDEPENDENT_ONLY = '{who}: supported likelihoods are BernoulliLikelihood, PoissonLikelihood and StudentTLikelihood, got _Other'
SOFTMAX_ONLY = ('{who}: supported for MulticlassSoftmax only, got {name}; the likelihoods with independent outputs have '
                'fit_q_newton_ (q_init="newton"), GaussianLikelihood has fit_q_')
DEEP = ('{who}: DeepRBFKernel is not supported (the feature map needs the gradient of the site pass for its inputs X, which the '
        'fused backward does not produce); {fit} supports it')
CLASSES = '{who}: at most 128 classes, got 129'
DAMPING = '{who}: damping must be in (0, 1], got {got}'
N_ITERS = '{who}: n_iters must be >= 0, got -1'
START = "{who}: start must be 'current' or 'prior', got 'best'"
ROUNDS = '{who}: n_rounds and m_steps must be >= 0, got {got}'
N_F = '{who}: n_f must be in [1, 65535], got {got}'
Y = '{who}: y must be int64 class indices of shape (40,), got {got}'
WEIGHTS = '{who}: weights must have shape (40,): one weight per point, got (3, 40)'
WEIGHTS_FIT = ('fit_q_softmax_: weights must have shape (40,): one weight per point (the classes of a point share one likelihood '
               'term), got (3, 40)')
NO_LIK = "{who}: params names 'lik', but {name} has no parameter"
SUBSET = '{who}: params must be a non-empty subset of {names}, got {got}'
LOO_LIK = ('loo: supported likelihoods are GaussianLikelihood, BernoulliLikelihood, PoissonLikelihood, StudentTLikelihood and '
           'MulticlassSoftmax, got _Other')


class _Other(torch.nn.Module):
    """A likelihood none of the families knows."""
    kind = 'other'


def refused(text, call, *args, **kwargs):
    with pytest.raises(ValueError, match='^' + re.escape(text) + '$'):
        call(*args, **kwargs)


@pytest.fixture(scope='module')
def m():
    """The models and the data, built once: nothing below changes them."""
    from vargp_amd.kernels import RBFKernel
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.vargp import VARGP
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, D, generator=g)
    labels = torch.arange(N) % C
    clf, counts, real = _Data(x, labels), _Data(x, torch.arange(N).float() % 4), _Data(x, torch.randn(N, generator=g))
    out = dict(x=x, labels=labels, clf=clf, counts=counts, real=real, wide=torch.ones(C, N),
               softmax=VARGP.create_clf(clf, M=M), bernoulli=VARGP.create_clf(clf, M=M, likelihood='bernoulli'),
               gauss=VARGP.create_reg(real, M=M), poisson=VARGP.create_reg(counts, M=M, likelihood='poisson'),
               studentt=VARGP.create_reg(real, M=M, likelihood='studentt'),
               softmax_noep=VARGP.create_clf(clf, M=M, ep_var_mean=False),
               bernoulli_noep=VARGP.create_clf(clf, M=M, likelihood='bernoulli', ep_var_mean=False),
               gauss_noep=VARGP.create_reg(real, M=M, ep_var_mean=False),
               softmax_deep=VARGP.create_clf(clf, M=M, dkl=True),
               bernoulli_deep=VARGP.create_clf(clf, M=M, dkl=True, likelihood='bernoulli'),
               many=VARGP(torch.randn(129, M, D, generator=g), RBFKernel(D), MulticlassSoftmax(n_f=10)))
    out['other'] = VARGP.create_clf(clf, M=M, likelihood='bernoulli')
    out['other'].likelihood = _Other()
    return out


# -- the model checks: likelihood in each direction, ep_var_mean, deep kernel, class cap -----------------------------------------------
INDEPENDENT = (('fit_q_newton_', False), ('site_bound', True), ('fit_sites_', True))
SOFTMAX = (('fit_q_softmax_', False), ('softmax_site_bound', True), ('fit_softmax_sites_', True))


@pytest.mark.parametrize('entry,differentiable', INDEPENDENT)
def test_independent_entries_refuse_the_model(m, entry, differentiable):
    x, y = m['x'], m['labels']
    refused(COUPLED.format(who=entry), getattr(m['softmax'], entry), x, y)
    refused(GAUSS.format(who=entry), getattr(m['gauss'], entry), x, y)
    refused(INDEPENDENT_ONLY.format(who=entry), getattr(m['other'], entry), x, y)
    refused(EP.format(who=entry), getattr(m['bernoulli_noep'], entry), x, y)
    if differentiable:                   # the deep kernel is refused FIRST: before the likelihood and ep_var_mean
        refused(DEEP.format(who=entry, fit='fit_q_newton_'), getattr(m['bernoulli_deep'], entry), x, y)
        refused(DEEP.format(who=entry, fit='fit_q_newton_'), getattr(m['softmax_deep'], entry), x, y)


@pytest.mark.parametrize('entry,differentiable', SOFTMAX)
def test_softmax_entries_refuse_the_model(m, entry, differentiable):
    x, y = m['x'], m['labels']
    for name, cls in (('bernoulli', 'BernoulliLikelihood'), ('gauss', 'GaussianLikelihood'), ('poisson', 'PoissonLikelihood'),
                      ('studentt', 'StudentTLikelihood'), ('other', '_Other')):
        refused(SOFTMAX_ONLY.format(who=entry, name=cls), getattr(m[name], entry), x, y)
    refused(EP.format(who=entry), getattr(m['softmax_noep'], entry), x, y)
    refused(CLASSES.format(who=entry), getattr(m['many'], entry), x, y)
    if differentiable:
        refused(DEEP.format(who=entry, fit='fit_q_softmax_'), getattr(m['softmax_deep'], entry), x, y)
        refused(DEEP.format(who=entry, fit='fit_q_softmax_'), getattr(m['bernoulli_deep'], entry), x, y)


def test_the_four_checkers(m):
    from vargp_amd import sites
    who = 'somebody'
    assert sites.check_supported(m['bernoulli']) is None and sites.check_supported(m['bernoulli_deep'], who) is None
    assert sites.check_differentiable(m['studentt'], who) is None
    assert sites.check_softmax_supported(m['softmax']) is None and sites.check_softmax_supported(m['softmax_deep'], who) is None
    assert sites.check_softmax_differentiable(m['softmax'], who) is None
    refused(COUPLED.format(who='fit_q_newton_'), sites.check_supported, m['softmax'])            # the default who
    refused(SOFTMAX_ONLY.format(who='fit_q_softmax_', name='PoissonLikelihood'), sites.check_softmax_supported, m['poisson'])
    for check, fit in ((sites.check_supported, None), (sites.check_differentiable, 'fit_q_newton_')):
        refused(COUPLED.format(who=who), check, m['softmax'], who)
        refused(GAUSS.format(who=who), check, m['gauss'], who)
        refused(INDEPENDENT_ONLY.format(who=who), check, m['other'], who)
        refused(EP.format(who=who), check, m['bernoulli_noep'], who)
        if fit:
            refused(DEEP.format(who=who, fit=fit), check, m['bernoulli_deep'], who)
    for check, fit in ((sites.check_softmax_supported, None), (sites.check_softmax_differentiable, 'fit_q_softmax_')):
        refused(SOFTMAX_ONLY.format(who=who, name='BernoulliLikelihood'), check, m['bernoulli'], who)
        refused(EP.format(who=who), check, m['softmax_noep'], who)
        refused(CLASSES.format(who=who), check, m['many'], who)
        if fit:
            refused(DEEP.format(who=who, fit=fit), check, m['softmax_deep'], who)


# -- the argument checks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entry,model', (('fit_q_newton_', 'bernoulli'), ('fit_q_softmax_', 'softmax')))
def test_fit_arguments(m, entry, model):
    fit, x, y = getattr(m[model], entry), m['x'], m['labels']
    for damping, got in ((0.0, '0.0'), (-0.5, '-0.5'), (1.5, '1.5'), (float('nan'), 'nan'), (2, '2.0')):
        refused(DAMPING.format(who=entry, got=got), fit, x, y, damping=damping)
    refused(N_ITERS.format(who=entry), fit, x, y, n_iters=-1)
    refused(START.format(who=entry), fit, x, y, start='best')
    refused(DAMPING.format(who=entry, got='0.0'), fit, x, y, damping=0.0, n_iters=-1, start='best')     # in this order
    refused(N_ITERS.format(who=entry), fit, x, y, n_iters=-1, start='best')


def test_fit_q_softmax_draws_and_weights(m):
    fit, x, y = m['softmax'].fit_q_softmax_, m['x'], m['labels']
    for n_f in (0, -1, 65536):
        refused(N_F.format(who='fit_q_softmax_', got=n_f), fit, x, y, n_f=n_f)
    refused(WEIGHTS_FIT, fit, x, y, weights=m['wide'])
    refused(START.format(who='fit_q_softmax_'), fit, x, y, start='best', n_f=0, weights=m['wide'])      # in this order
    refused(N_F.format(who='fit_q_softmax_', got=0), fit, x, y, n_f=0, weights=m['wide'])
    refused(WEIGHTS_FIT, fit, x, y.float(), weights=m['wide'])          # (the fit checks y with its targets, on the device)


@pytest.mark.parametrize('entry', ('softmax_site_bound', 'fit_softmax_sites_', 'loo'))
def test_softmax_data_and_draws(m, entry):
    call, x, y = getattr(m['softmax'], entry), m['x'], m['labels']
    for n_f in (0, -1, 65536):
        refused(N_F.format(who=entry, got=n_f), call, x, y, n_f=n_f)
    refused(Y.format(who=entry, got='torch.float32 (40,)'), call, x, y.float())
    refused(Y.format(who=entry, got='torch.int32 (40,)'), call, x, y.int())
    refused(Y.format(who=entry, got='torch.int64 (39,)'), call, x, y[:39])
    refused(Y.format(who=entry, got='torch.int64 (3, 40)'), call, x, y.expand(C, N))
    refused(WEIGHTS.format(who=entry), call, x, y, weights=m['wide'])
    refused(N_F.format(who=entry, got=0), call, x, y.float(), weights=m['wide'], n_f=0)                 # in this order
    refused(Y.format(who=entry, got='torch.float32 (40,)'), call, x, y.float(), weights=m['wide'])


def test_em_arguments(m):
    x, y = m['x'], m['labels']
    for entry, model in (('fit_sites_', 'bernoulli'), ('fit_softmax_sites_', 'softmax')):
        em = getattr(m[model], entry)
        for damping, got in ((0.0, '0.0'), (1.5, '1.5'), (float('nan'), 'nan')):
            refused(DAMPING.format(who=entry, got=got), em, x, y, damping=damping)
        refused(ROUNDS.format(who=entry, got='-1, 20'), em, x, y, n_rounds=-1)
        refused(ROUNDS.format(who=entry, got='5, -2'), em, x, y, m_steps=-2)
        refused(DAMPING.format(who=entry, got='0.0'), em, x, y, damping=0.0, n_rounds=-1)               # in this order
    refused(ROUNDS.format(who='fit_softmax_sites_', got='-1, 20'), m['softmax'].fit_softmax_sites_, x, y, n_rounds=-1, n_f=0)
    refused(N_F.format(who='fit_softmax_sites_', got=0), m['softmax'].fit_softmax_sites_, x, y.float(), n_f=0)


def test_em_params(m):
    x, y = m['x'], m['labels']
    em, names = m['bernoulli'].fit_sites_, "['kernel', 'lik', 'z']"
    refused(NO_LIK.format(who='fit_sites_', name='BernoulliLikelihood'), em, x, y, params=('z', 'lik'))
    refused(NO_LIK.format(who='fit_sites_', name='PoissonLikelihood'), m['poisson'].fit_sites_, x, y, params=['lik'])
    refused(SUBSET.format(who='fit_sites_', names=names, got='()'), em, x, y, params=())
    refused(SUBSET.format(who='fit_sites_', names=names, got="('z', 'noise')"), em, x, y, params=('z', 'noise'))
    refused(SUBSET.format(who='fit_sites_', names=names, got="('lik', 'noise')"), em, x, y, params=('lik', 'noise'))
    refused(NO_LIK.format(who='fit_sites_', name='BernoulliLikelihood'), em, x, y, params=('lik',), damping=0.0)
    refused(SUBSET.format(who='fit_sites_', names=names, got="('noise',)"), m['studentt'].fit_sites_, x, y, params=('noise',))
    em, names = m['softmax'].fit_softmax_sites_, "['kernel', 'z']"
    refused(NO_LIK.format(who='fit_softmax_sites_', name='MulticlassSoftmax'), em, x, y, params=('z', 'lik'))
    refused(NO_LIK.format(who='fit_softmax_sites_', name='MulticlassSoftmax'), em, x, y, params=('lik', 'noise'))
    refused(SUBSET.format(who='fit_softmax_sites_', names=names, got='()'), em, x, y, params=())
    refused(SUBSET.format(who='fit_softmax_sites_', names=names, got="('z', 'noise')"), em, x, y, params=('z', 'noise'))
    refused(SUBSET.format(who='fit_softmax_sites_', names=names, got="('noise',)"), em, x, y, params=('noise',), damping=0.0)


def test_loo(m):
    x, y = m['x'], m['labels']
    refused(LOO_LIK, m['other'].loo, x, y)
    for model in ('softmax_noep', 'bernoulli_noep', 'gauss_noep'):
        refused(EP.format(who='loo'), m[model].loo, x, y)
    refused(CLASSES.format(who='loo'), m['many'].loo, x, y)
    for model in ('softmax', 'bernoulli', 'gauss'):
        refused('loo: tile must be >= 1, got 0', m[model].loo, x, y, tile=0)
    refused('loo: tile must be >= 1, got 0', m['softmax'].loo, x, y, tile=0, n_f=0)                     # in this order


# -- the factories: every q_init x likelihood ------------------------------------------------------------------------------------------
CLF_COUPLED = ("create_clf: q_init={q!r} fits independent Gaussian sites, which likelihood='softmax' does not have (its outputs are "
               "coupled); use likelihood='bernoulli'")
CLF_NEWTON_SOFTMAX = ("create_clf: q_init='newton_softmax' fits the coupled sites of likelihood='softmax', got 'bernoulli'; the "
                      "likelihoods with independent outputs have q_init='newton'")
CLF_EM_SOFTMAX = ("create_clf: q_init='em_softmax' is variational EM on the coupled sites of likelihood='softmax', got 'bernoulli'; "
                  "the likelihoods with independent outputs have q_init='em'")
REG_CLOSED = "create_reg: q_init={q!r} is the closed form of likelihood='gaussian', got {lik!r}"
REG_SITES = ("create_reg: q_init={q!r} iterates Gaussian sites of a non-Gaussian likelihood ('poisson', 'studentt'); "
             "likelihood='gaussian' has the closed form q_init='optimal'")


def test_factory_q_init_names(m):
    from vargp_amd.vargp import VARGP, _CLF_Q_INITS, _Q_INITS
    assert _CLF_Q_INITS == ('default', 'newton', 'em', 'newton_softmax', 'em_softmax')
    assert _Q_INITS == ('default', 'optimal', 'collapsed', 'newton', 'em')
    for q in ('optimal', 'collapsed', 'best'):
        refused(f"create_clf: q_init must be one of ['default', 'em', 'em_softmax', 'newton', 'newton_softmax'], got {q!r}",
                VARGP.create_clf, m['clf'], M=M, q_init=q)
    for q in ('newton_softmax', 'em_softmax', 'best'):
        refused(f"create_reg: q_init must be one of ['collapsed', 'default', 'em', 'newton', 'optimal'], got {q!r}",
                VARGP.create_reg, m['real'], M=M, q_init=q)
    refused("create_clf: q_init must be one of ['default', 'em', 'em_softmax', 'newton', 'newton_softmax'], got 'best'",
            VARGP.create_clf, m['clf'], M=M, q_init='best', likelihood='gaussian', kernel='cubic')     # q_init is judged first
    refused("create_reg: q_init must be one of ['collapsed', 'default', 'em', 'newton', 'optimal'], got 'best'",
            VARGP.create_reg, m['real'], M=M, q_init='best', likelihood='softmax', kernel='cubic')


def test_factory_q_init_against_likelihood(m):
    from vargp_amd.vargp import VARGP
    for q in ('newton', 'em'):
        refused(CLF_COUPLED.format(q=q), VARGP.create_clf, m['clf'], M=M, q_init=q)
        refused(CLF_COUPLED.format(q=q), VARGP.create_clf, m['clf'], M=M, q_init=q, likelihood='softmax', kernel='cubic')
        refused(REG_SITES.format(q=q), VARGP.create_reg, m['real'], M=M, q_init=q)
        refused(REG_SITES.format(q=q), VARGP.create_reg, m['real'], M=M, q_init=q, kernel='cubic', z_init='best')
    refused(CLF_NEWTON_SOFTMAX, VARGP.create_clf, m['clf'], M=M, q_init='newton_softmax', likelihood='bernoulli')
    refused(CLF_EM_SOFTMAX, VARGP.create_clf, m['clf'], M=M, q_init='em_softmax', likelihood='bernoulli', z_init='best')
    for q in ('optimal', 'collapsed'):
        for lik in ('poisson', 'studentt'):
            data = m['counts'] if lik == 'poisson' else m['real']
            refused(REG_CLOSED.format(q=q, lik=lik), VARGP.create_reg, data, M=M, q_init=q, likelihood=lik)
        refused(REG_CLOSED.format(q=q, lik='cauchy'), VARGP.create_reg, m['real'], M=M, q_init=q, likelihood='cauchy')
    # an unknown likelihood is named by the q_init check where that comes first, by the likelihood's own otherwise
    refused("create_clf: q_init='newton' fits independent Gaussian sites, which likelihood='probit' does not have (its outputs are "
            "coupled); use likelihood='bernoulli'", VARGP.create_clf, m['clf'], M=M, q_init='newton', likelihood='probit')
    refused("create_reg: likelihood must be 'gaussian', 'studentt' or 'poisson', got 'cauchy'",
            VARGP.create_reg, m['real'], M=M, q_init='newton', likelihood='cauchy')


def test_factory_q_init_checks_the_model_before_any_device_work(m):
    from vargp_amd.vargp import VARGP
    for q, lik in (('newton', 'bernoulli'), ('em', 'bernoulli'), ('newton_softmax', 'softmax'), ('em_softmax', 'softmax')):
        refused(EP.format(who=f'create_clf(q_init="{q}")'), VARGP.create_clf, m['clf'], M=M, q_init=q, likelihood=lik, ep_var_mean=False)
    refused(DEEP.format(who='create_clf(q_init="em")', fit='fit_q_newton_'),
            VARGP.create_clf, m['clf'], M=M, q_init='em', likelihood='bernoulli', dkl=True)
    refused(DEEP.format(who='create_clf(q_init="em_softmax")', fit='fit_q_softmax_'),
            VARGP.create_clf, m['clf'], M=M, q_init='em_softmax', dkl=True)
    for q, lik in (('optimal', 'gaussian'), ('collapsed', 'gaussian'), ('newton', 'poisson'), ('em', 'studentt')):
        data = m['counts'] if lik == 'poisson' else m['real']
        refused(EP.format(who=f'create_reg(q_init="{q}")'), VARGP.create_reg, data, M=M, q_init=q, likelihood=lik, ep_var_mean=False)


def test_experiment_driver_offers_the_factory_q_inits():
    import importlib.util
    import os
    from vargp_amd.vargp import _CLF_Q_INITS
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'experiments', 'vargp.py')
    spec = importlib.util.spec_from_file_location('experiments_vargp_driver', path)
    driver = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(driver)
    for cmd in ('toy', 's-mnist', 'p-mnist'):
        for q in _CLF_Q_INITS:
            assert driver.parse_args([cmd, '--q_init', q]).q_init == q
        with pytest.raises(SystemExit):
            driver.parse_args([cmd, '--q_init', 'optimal'])
