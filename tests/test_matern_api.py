"""CPU: the Matern kernel's Python surface -- both package names, argument validation, state dict, no CPU fallback,
create_clf(kernel=) and the driver's --kernel flag."""
import pytest
import torch


def test_import_under_both_package_names():
    import var_gp.kernels
    import vargp_amd.kernels
    assert var_gp.kernels.MaternKernel is vargp_amd.kernels.MaternKernel
    assert issubclass(vargp_amd.kernels.MaternKernel, vargp_amd.kernels.RBFKernel)


@pytest.mark.parametrize('nu', [0.5, 1.5, 2.5])
def test_accepted_nu(nu):
    from vargp_amd.kernels import MaternKernel
    assert MaternKernel(3, nu=nu).nu == nu
    assert MaternKernel(3).nu == 2.5


@pytest.mark.parametrize('nu', [0, 1, 2.0, 3.5, float('inf'), None, '1.5'])
def test_bad_nu_raises(nu):
    from vargp_amd import ops
    from vargp_amd.kernels import MaternKernel
    with pytest.raises(ValueError):
        MaternKernel(3, nu=nu)
    with pytest.raises(ValueError):
        ops.matern_gram(torch.zeros(1, 3), torch.zeros(1, 4, 2), nu=nu)


def test_state_dict_keys_equal_rbf_and_nu_is_not_state():
    from vargp_amd.kernels import MaternKernel, RBFKernel
    m, r = MaternKernel(5, nu=1.5), RBFKernel(5)
    assert list(m.state_dict()) == list(r.state_dict())
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in r.named_parameters()]
    other = MaternKernel(5, nu=0.5)
    other.load_state_dict(m.state_dict())
    assert other.nu == 0.5
    r.load_state_dict(m.state_dict())            # interchangeable with the RBF's


def test_constructor_arguments_reach_the_base_class():
    from vargp_amd.kernels import MaternKernel
    pm, pv = torch.randn(4), torch.randn(4)
    k = MaternKernel(3, 0.5, pm, pv, True)
    assert k.map_est and torch.equal(k.prior_log_mean, pm) and torch.equal(k.prior_log_logvar, pv)
    assert k.compute_diag(torch.zeros(2, 4)).shape == (2, 1, 1)


def test_no_cpu_fallback():
    from vargp_amd import ops
    from vargp_amd._lib import VargpHipError
    from vargp_amd.kernels import MaternKernel
    for nu in (0.5, 1.5, 2.5):
        with pytest.raises(VargpHipError):
            ops.matern_gram(torch.zeros(1, 3), torch.zeros(1, 4, 2), nu=nu)
        with pytest.raises(VargpHipError):
            ops.matern_gram(torch.zeros(1, 3), torch.zeros(1, 4, 2), torch.zeros(5, 2), True, nu)
        with pytest.raises(VargpHipError):
            MaternKernel(2, nu=nu).compute(torch.zeros(1, 3), torch.zeros(2, 4, 2))


def test_create_clf_kernel_keyword():
    from vargp_amd.datasets import ToyDataset
    from vargp_amd.kernels import DeepRBFKernel, MaternKernel, RBFKernel
    from vargp_amd.vargp import VARGP
    ds = ToyDataset()
    assert type(VARGP.create_clf(ds, M=4).kernel) is RBFKernel
    assert type(VARGP.create_clf(ds, M=4, kernel='rbf').kernel) is RBFKernel
    assert type(VARGP.create_clf(ds, M=4, dkl=True, kernel='rbf').kernel) is DeepRBFKernel
    for name, nu in (('matern12', 0.5), ('matern32', 1.5), ('matern52', 2.5)):
        k = VARGP.create_clf(ds, M=4, kernel=name, map_est_hypers=True).kernel
        assert type(k) is MaternKernel and k.nu == nu and k.map_est
        with pytest.raises(ValueError):
            VARGP.create_clf(ds, M=4, dkl=True, kernel=name)
    for bad in ('matern', 'matern72', 'RBF', None, 1.5):
        with pytest.raises(ValueError):
            VARGP.create_clf(ds, M=4, kernel=bad)


def test_create_clf_hands_the_hyper_posterior_to_a_matern_prior():
    from vargp_amd.datasets import ToyDataset
    from vargp_amd.kernels import MaternKernel
    from vargp_amd.vargp import VARGP
    ds = ToyDataset()
    gp0 = VARGP.create_clf(ds, M=4, kernel='matern52')
    sd = {k: v.clone() for k, v in gp0.state_dict().items()}
    gp1 = VARGP.create_clf(ds, M=4, kernel='matern52', prev_params=[sd])
    assert type(gp1.kernel) is MaternKernel
    assert torch.equal(gp1.kernel.prior_log_mean, gp0.kernel.log_mean.detach())
    assert torch.equal(gp1.kernel.prior_log_logvar, gp0.kernel.log_logvar.detach())
    assert not any(k.startswith('kernel') for k in sd)           # popped, as for the RBF


def test_matern_model_is_never_routed_to_a_native_program():
    from vargp_amd.datasets import ToyDataset
    from vargp_amd.vargp import VARGP
    gp = VARGP.create_clf(ToyDataset(), M=4, kernel='matern32')
    assert not gp._use_block_program(32) and not gp._tn_applicable()


def test_driver_has_a_kernel_flag():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('exp_vargp', os.path.join(ROOT, 'experiments', 'vargp.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit):
        mod.main(['toy', '--kernel', 'matern72'])
