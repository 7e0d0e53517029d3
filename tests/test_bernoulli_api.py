"""CPU: BernoulliLikelihood (independent outputs: binary, multi-label, one-vs-rest; not in the reference) -- the class and its
helpers, the C-ABI symbols of csrc/indep_lik.hip, target conversion, create_clf(likelihood=) and the driver's flags."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = {'vargp_bernoulli_workspace_bytes': 3, 'vargp_bernoulli_nll_fwd': 13, 'vargp_bernoulli_nll_bwd': 16,
           'vargp_bernoulli_predict': 8}


def test_symbols_declared_exported_bound():
    from vargp_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vargp_hip.h')).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in SYMBOLS.items():
        assert re.search(rf'\b{name}\s*\(', text), name
        assert hasattr(handle, name), name
        assert name in _lib.EXPORTS and len(_lib._SIGNATURES[name][1]) == nargs, name
    assert _lib._SIGNATURES['vargp_bernoulli_workspace_bytes'][0] is ctypes.c_size_t
    # ldt is 64-bit, the link an int, the workspace size a size_t
    fwd = _lib._SIGNATURES['vargp_bernoulli_nll_fwd'][1]
    assert fwd[3] is ctypes.c_int64 and fwd[5] is ctypes.c_int and fwd[11] is ctypes.c_size_t


def test_header_says_not_in_the_reference():
    text = open(os.path.join(ROOT, 'include', 'vargp_hip.h')).read()
    block = text[text.index('Independent-output Bernoulli likelihood'):text.index('vargp_bernoulli_predict')]
    assert 'Not in the reference' in block


def test_class_has_no_parameters_and_no_n_f():
    from var_gp.likelihoods import BernoulliLikelihood
    from vargp_amd.likelihoods import BernoulliLikelihood as B2
    assert BernoulliLikelihood is B2
    lik = BernoulliLikelihood()
    assert lik.link == 'probit' and BernoulliLikelihood(link='logit').link == 'logit'
    assert list(lik.parameters()) == [] and list(lik.buffers()) == [] and lik.state_dict() == {}
    assert not hasattr(lik, 'n_f')
    assert lik.ext_param() is None
    with pytest.raises(ValueError):
        BernoulliLikelihood(link='cloglog')
    for line in ('<= 3e-4 (probit) and <= 3e-6 (logit)', 'at var <= 25 it is 5e-3', 'SUMS over outputs'):
        assert line in BernoulliLikelihood.__doc__, line
    assert 'NOT normalised' in BernoulliLikelihood.predict.__doc__


def test_n_f_is_external_is_gaussian():
    from vargp_amd.likelihoods import BernoulliLikelihood, GaussianLikelihood, MulticlassSoftmax, is_external, is_gaussian, n_f
    b, g, s = BernoulliLikelihood(), GaussianLikelihood(3), MulticlassSoftmax(n_f=7)
    assert (n_f(b), n_f(g), n_f(s)) == (1, 1, 7)
    assert is_external(b) and is_external(g) and not is_external(s)
    assert not is_gaussian(b) and is_gaussian(g) and not is_gaussian(s)
    for lik in (b, g):
        assert all(hasattr(lik, m) for m in ('ext_param', 'ext_target', 'ext_value', 'ext_backward'))
    assert g.ext_param() is g.obs_log_var


def test_model_state_dict_has_no_likelihood_entry():
    from vargp_amd.kernels import RBFKernel
    from vargp_amd.likelihoods import BernoulliLikelihood
    from vargp_amd.vargp import VARGP
    gp = VARGP(torch.randn(3, 5, 2), RBFKernel(2), BernoulliLikelihood(), n_var_samples=2)
    assert not [k for k in gp.state_dict() if k.startswith('likelihood')]
    assert gp.draw_t0_noise(torch.zeros(4, 2))[1] is None          # no eps_f
    assert not gp._lazy_ok()


def test_bernoulli_target_accepts():
    from vargp_amd.ops import bernoulli_target
    C, B = 3, 5
    y = torch.tensor([0, 2, 1, 7, -1])
    t, ldt, labels = bernoulli_target(y, C, B)
    assert t is None and ldt == 0 and labels.dtype == torch.int64 and torch.equal(labels, y)
    for dtype in (torch.float32, torch.float64, torch.float16, torch.bool):
        m = (torch.arange(C * B).reshape(C, B) % 2).to(dtype)
        t, ldt, labels = bernoulli_target(m, C, B)
        assert labels is None and ldt == B and t.dtype == torch.float32 and t.is_contiguous()
        assert torch.equal(t, m.float())
        t, ldt, labels = bernoulli_target(m[0], C, B)
        assert labels is None and ldt == 0 and tuple(t.shape) == (B,) and t.dtype == torch.float32
    t, ldt, _ = bernoulli_target(torch.ones(B, C).t(), C, B)        # a transposed view is made contiguous
    assert t.is_contiguous() and ldt == B
    t, _, _ = bernoulli_target(torch.ones(C, B, requires_grad=True), C, B)
    assert not t.requires_grad


def test_bernoulli_target_rejects():
    from vargp_amd.ops import bernoulli_target
    C, B = 3, 5
    for bad in (torch.zeros(C, B, dtype=torch.int64), torch.zeros(B + 1, dtype=torch.int64), torch.zeros((), dtype=torch.int64)):
        with pytest.raises(ValueError):
            bernoulli_target(bad, C, B)
    for bad in (torch.zeros(B, C), torch.zeros(B + 1), torch.zeros(1, C, B), torch.zeros(C, B + 1, dtype=torch.bool)):
        with pytest.raises(ValueError):
            bernoulli_target(bad, C, B)
    for dtype in (torch.int32, torch.uint8, torch.int16, torch.complex64):
        with pytest.raises(TypeError):
            bernoulli_target(torch.zeros(B, dtype=dtype), C, B)
    with pytest.raises(TypeError):
        bernoulli_target([0, 1, 2, 0, 1], C, B)


def test_ops_refuse_cpu_tensors_and_unknown_links():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    mu, var = torch.zeros(1, 2, 3), torch.ones(1, 2, 3)
    with pytest.raises(VargpHipError):
        ops.bernoulli_nll(mu, var, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(VargpHipError):
        ops.bernoulli_predict(mu, var)
    with pytest.raises(ValueError):
        ops.bernoulli_nll(mu, var, torch.zeros(3, dtype=torch.int64), link='cloglog')
    assert ops.BERNOULLI_LINKS == {'probit': 0, 'logit': 1}


def test_create_clf_likelihood_choice():
    from vargp_amd.datasets import ToyDataset
    from vargp_amd.kernels import DeepRBFKernel, MaternKernel
    from vargp_amd.likelihoods import BernoulliLikelihood, MulticlassSoftmax
    from vargp_amd.vargp import VARGP
    from vargp_amd.vargp_retrain import VARGPRetrain
    ds = ToyDataset()
    gp = VARGP.create_clf(ds, M=4, n_f=6)
    assert type(gp.likelihood) is MulticlassSoftmax and gp.likelihood.n_f == 6          # the default is unchanged
    assert type(VARGP.create_clf(ds, M=4, likelihood='softmax').likelihood) is MulticlassSoftmax
    gp = VARGP.create_clf(ds, M=4, likelihood='bernoulli')
    assert type(gp.likelihood) is BernoulliLikelihood and gp.likelihood.link == 'probit'
    gp = VARGP.create_clf(ds, M=4, likelihood='bernoulli', link='logit', kernel='matern32', native_kernel=True)
    assert gp.likelihood.link == 'logit' and type(gp.kernel) is MaternKernel
    gp = VARGP.create_clf(ds, M=4, likelihood='bernoulli', dkl=True)
    assert type(gp.likelihood) is BernoulliLikelihood and type(gp.kernel) is DeepRBFKernel
    for bad in (dict(likelihood='gaussian'), dict(likelihood='Bernoulli'), dict(likelihood=None),
                dict(likelihood='bernoulli', link='cloglog')):
        with pytest.raises(ValueError):
            VARGP.create_clf(ds, M=4, **bad)
    # not part of a checkpoint: the state dicts of the two choices have the same keys
    a, b = VARGP.create_clf(ds, M=4), VARGP.create_clf(ds, M=4, likelihood='bernoulli')
    assert set(a.state_dict()) == set(b.state_dict())
    r = VARGPRetrain.create_clf(ds, M=4, likelihood='bernoulli', link='logit')
    assert type(r.likelihood) is BernoulliLikelihood and r.likelihood.link == 'logit'
    assert type(VARGPRetrain.create_clf(ds, M=4).likelihood) is MulticlassSoftmax
    with pytest.raises(ValueError):
        VARGPRetrain.create_clf(ds, M=4, likelihood='probit')


def _driver():
    import importlib.util
    spec = importlib.util.spec_from_file_location('vargp_driver', os.path.join(ROOT, 'experiments', 'vargp.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('cmd', ['toy', 's-mnist', 'p-mnist'])
def test_driver_flags(cmd, capsys):
    drv = _driver()
    a = drv.parse_args([cmd])
    assert a.likelihood == 'softmax' and a.link == 'probit'
    a = drv.parse_args([cmd, '--likelihood', 'bernoulli', '--link', 'logit', '--kernel', 'matern52'])
    assert a.likelihood == 'bernoulli' and a.link == 'logit'
    assert drv.parse_args([cmd, '--graph']).graph                     # softmax + --graph stays legal
    for bad in (['--likelihood', 'gaussian'], ['--link', 'cloglog']):
        with pytest.raises(SystemExit):
            drv.parse_args([cmd] + bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        drv.parse_args([cmd, '--likelihood', 'bernoulli', '--graph'])
    err = capsys.readouterr().err
    assert 'epoch graphs' in err and 'refuse' in err


def test_driver_retrain_takes_the_likelihood():
    drv = _driver()
    a = drv.parse_args(['toy', '--retrain', '--likelihood', 'bernoulli'])
    assert a.retrain and a.likelihood == 'bernoulli'
    import inspect
    sig = inspect.signature(drv.train)
    assert sig.parameters['likelihood'].default == 'softmax' and sig.parameters['link'].default == 'probit'
