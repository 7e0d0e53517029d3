"""CPU: the reference's GaussianLikelihood (var_gp/likelihoods.py:66-110) exists under both package names with the reference's
constructor, parameter and state-dict key, and its two C-ABI kernels are declared, exported and bound."""
import ctypes
import inspect
import os
import re

import torch

from conftest import ROOT


def test_import_through_reference_name():
    from var_gp.likelihoods import GaussianLikelihood
    from vargp_amd.likelihoods import GaussianLikelihood as G2
    assert GaussianLikelihood is G2


def test_constructor_parameter_and_state_dict_key():
    from var_gp.likelihoods import GaussianLikelihood
    from var_gp.kernels import RBFKernel
    from var_gp.vargp import VARGP
    sig = inspect.signature(GaussianLikelihood.__init__)
    assert list(sig.parameters) == ['self', 'out_size', 'init_log_var']
    assert sig.parameters['init_log_var'].default == -4.0
    lik = GaussianLikelihood(7)
    assert [n for n, _ in lik.named_parameters()] == ['obs_log_var']
    assert lik.obs_log_var.shape == (7,) and lik.obs_log_var.requires_grad
    assert torch.equal(lik.obs_log_var.detach(), torch.full((7,), -4.0))
    assert torch.equal(GaussianLikelihood(3, init_log_var=-1.5).obs_log_var.detach(), torch.full((3,), -1.5))
    gp = VARGP(torch.randn(3, 5, 2), RBFKernel(2), GaussianLikelihood(3), n_var_samples=2)
    sd = gp.state_dict()
    assert 'likelihood.obs_log_var' in sd and sd['likelihood.obs_log_var'].shape == (3,)
    # a task-0 model's state_dict() is a valid prev_params entry (extra keys ignored, reference vargp.py:17-20)
    gp1 = VARGP(torch.randn(3, 5, 2), RBFKernel(2), GaussianLikelihood(3), prev_params=[sd])
    assert set(gp1.prev_params[0]) == {'z', 'u_mean', 'u_tril_vec'}


def test_forward_and_predict_shapes():
    from var_gp.likelihoods import GaussianLikelihood
    lik = GaussianLikelihood(4, init_log_var=-2.0)
    mu, var = torch.randn(3, 4, 6), torch.rand(3, 4, 6)
    om, ov = lik(mu, var)
    assert om.shape == (3, 4, 6, 1) and ov.shape == (3, 4, 6, 1)
    torch.testing.assert_close(ov[..., 0], var + torch.exp(torch.tensor(-2.0)))
    assert lik.predict(mu, var) is mu


def test_programs_see_one_sample_per_hyper_sample():
    from vargp_amd.likelihoods import GaussianLikelihood, MulticlassSoftmax, n_f
    assert n_f(GaussianLikelihood(3)) == 1
    assert n_f(MulticlassSoftmax(n_f=7)) == 7
    assert not hasattr(GaussianLikelihood(3), 'n_f')


def test_gauss_symbols_declared_exported_bound():
    from vargp_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'vargp_hip.h')).read(), flags=re.S)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('vargp_gauss_nll_fwd', 'vargp_gauss_nll_bwd'):
        assert re.search(rf'\b{name}\s*\(', text), name
        assert hasattr(handle, name), name
        assert name in _lib._SIGNATURES
    assert len(_lib._SIGNATURES['vargp_gauss_nll_fwd'][1]) == 10
    assert len(_lib._SIGNATURES['vargp_gauss_nll_bwd'][1]) == 14


def test_gauss_op_refuses_cpu_tensors():
    import pytest
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    with pytest.raises(VargpHipError):
        ops.gauss_nll(torch.zeros(1, 2, 3), torch.ones(1, 2, 3), torch.zeros(2, 3), torch.zeros(2))
