"""CPU: the interface of the opt-in native route of MaternKernel models -- what the library exports for it, the one predicate
that decides the route, the constructor / factory / driver arguments, and that the ctypes mirror of vargp_elbo_tn_desc and
include/vargp_hip.h agree on its size.  (What the route computes is tested on the GPU: tests/test_hip_matern_native.py.)"""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_and_descriptor_field():
    from vargp_amd import _lib
    lib = _lib.lib()
    assert 'vargp_elbo_tn_desc_bytes' in _lib.EXPORTS and hasattr(lib, 'vargp_elbo_tn_desc_bytes')
    assert _lib.ElboTnDesc._fields_[-1] == ('kernel_nu2', ctypes.c_int32)
    # the struct as the library was compiled == its ctypes mirror
    assert lib.vargp_elbo_tn_desc_bytes() == ctypes.sizeof(_lib.ElboTnDesc)
    assert _lib.ElboTnDesc().kernel_nu2 == 0                  # a zero-initialised descriptor is the RBF program


def test_header_and_ctypes_agree_on_the_descriptor_size(tmp_path):
    from vargp_amd import _lib
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or '/opt/rocm/llvm/bin/clang'
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vargp_hip.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(vargp_elbo_tn_desc), offsetof(vargp_elbo_tn_desc, kernel_nu2)); return 0; }\n')
    exe = tmp_path / 'size'
    subprocess.check_call([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    size, off = map(int, subprocess.check_output([str(exe)]).split())
    assert size == ctypes.sizeof(_lib.ElboTnDesc) and off == _lib.ElboTnDesc.kernel_nu2.offset


@pytest.mark.parametrize('entry,nargs', [('vargp_elbo_tn_fwd', 1), ('vargp_elbo_tn_begin', 1), ('vargp_elbo_tn_bwd', 7),
                                         ('vargp_elbo_tn_end', 7), ('vargp_elbo_tn_hyper_desc', 2)])
def test_library_rejects_an_unknown_kernel_code(entry, nargs):
    """kernel_nu2 = 2 is refused before anything is launched (no GPU is touched: the check comes first)."""
    from vargp_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = _lib.ElboTnDesc(S=1, C=1, M=4, D=2, B=4, F=1, nblk=1, map_est=1, jitter=1e-4, kernel_nu2=2, ws=p, ws_bytes=64)
    args = [p] * nargs
    if entry == 'vargp_elbo_tn_hyper_desc':
        args = [p, ctypes.byref(_lib.HyperGradDesc())]
    rc = getattr(lib, entry)(ctypes.byref(d), *args)
    assert rc != 0 and b'kernel_nu2 = 2' in lib.vargp_last_error()


def test_moments_tile_and_lik_buffers_reject_an_unknown_kernel_code():
    from vargp_amd import _lib
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    d = _lib.ElboTnDesc(S=1, C=1, M=4, D=2, B=4, F=1, nblk=1, kernel_nu2=4, ws=p, ws_bytes=64)
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.vargp_elbo_tn_moments(ctypes.byref(d), ctypes.byref(a), ctypes.byref(b)) != 0
    assert b'kernel_nu2 = 4' in lib.vargp_last_error()
    assert lib.vargp_elbo_tn_tile(ctypes.byref(d), p, p, p, p, 4, None) != 0 and b'kernel_nu2 = 4' in lib.vargp_last_error()
    assert lib.vargp_elbo_tn_lik_buffers(ctypes.byref(d), None, None, None, None) != 0 and b'kernel_nu2 = 4' in lib.vargp_last_error()


def test_workspace_sizes_do_not_depend_on_the_kernel():
    """The Matern backward recomputes d2 into buffers that are dead by then: no `_k` variants of the size queries."""
    from vargp_amd import _lib
    assert not [n for n in _lib.EXPORTS if n.startswith('vargp_elbo_tn_workspace_bytes') and n.endswith('_k')]


def test_native_is_a_constructor_argument_not_state():
    from vargp_amd.kernels import MaternKernel, RBFKernel
    torch.manual_seed(0)
    a = MaternKernel(5, nu=1.5, native=True)
    assert a.native is True and MaternKernel(5).native is False
    b, r = MaternKernel(5, nu=1.5), RBFKernel(5)
    assert set(a.state_dict()) == set(b.state_dict()) == set(r.state_dict())
    b.load_state_dict(a.state_dict())
    r.load_state_dict(a.state_dict())
    a.load_state_dict(r.state_dict())
    assert torch.equal(b.log_mean, a.log_mean) and torch.equal(r.log_mean, a.log_mean)
    assert a.native is True and b.native is False


def test_route_predicate():
    from vargp_amd.kernels import DeepRBFKernel, MaternKernel, RBFKernel, native_code

    class Sub(RBFKernel):
        pass

    class SubM(MaternKernel):
        pass

    assert native_code(RBFKernel(3)) == 0
    assert [native_code(MaternKernel(3, nu=nu, native=True)) for nu in (0.5, 1.5, 2.5)] == [1, 3, 5]
    assert native_code(MaternKernel(3, nu=2.5)) is None
    assert native_code(DeepRBFKernel(3)) is None and native_code(Sub(3)) is None and native_code(SubM(3, native=True)) is None


def test_model_routing_follows_the_predicate():
    """_use_block_program on the host (the device test is part of _tn_applicable: replaced by the predicate alone here)."""
    from vargp_amd.kernels import MaternKernel, native_code
    from vargp_amd.likelihoods import MulticlassSoftmax
    from vargp_amd.vargp import VARGP

    class OnDevice(VARGP):
        def _tn_applicable(self):
            return self.fused_tasks and native_code(self.kernel) is not None

    z = torch.randn(2, 6, 3)
    for native in (True, False):
        gp = OnDevice(z, MaternKernel(3, nu=0.5, native=native), MulticlassSoftmax(n_f=2))
        assert not VARGP._tn_applicable(gp)                                  # CPU tensors: never
        assert not gp.first_task_as_block(64)                                # M = 6: the RBF rule says first-task program
        assert bool(gp._use_block_program(64)) == native                     # ... which a native Matern model never takes
        gp.fused_first_task = False
        assert not gp._use_block_program(64)                                 # cleared: composed route


def test_tn_program_refuses_unknown_codes():
    from vargp_amd.fused import TnProgram
    with pytest.raises(ValueError, match='kernel_nu2'):
        TnProgram(1, 1, 4, 2, 4, 1, 1, 'cpu', kernel_nu2=2)


def test_create_clf_native_kernel_argument():
    from vargp_amd.datasets import ToyDataset
    from vargp_amd.kernels import MaternKernel, native_code
    from vargp_amd.vargp import VARGP
    ds = ToyDataset()
    gp = VARGP.create_clf(ds, M=4, n_f=2, kernel='matern52', native_kernel=True)
    assert type(gp.kernel) is MaternKernel and gp.kernel.native and native_code(gp.kernel) == 5
    assert native_code(VARGP.create_clf(ds, M=4, n_f=2, kernel='matern52').kernel) is None
    with pytest.raises(ValueError, match='native_kernel'):
        VARGP.create_clf(ds, M=4, n_f=2, kernel='rbf', native_kernel=True)
    with pytest.raises(ValueError, match='native_kernel'):
        VARGP.create_clf(ds, M=4, n_f=2, dkl=True, native_kernel=True)


def test_driver_parses_native_kernel(capsys):
    sys.path.insert(0, os.path.join(ROOT, 'experiments'))
    try:
        import vargp as driver
    finally:
        sys.path.pop(0)
    args = driver.parse_args(['toy', '--kernel', 'matern32', '--native_kernel'])
    assert args.native_kernel is True and args.kernel == 'matern32'
    assert driver.parse_args(['toy', '--kernel', 'matern32']).native_kernel is False
    for bad in (['toy', '--native_kernel'], ['s-mnist', '--kernel', 'matern12', '--dkl', '1', '--native_kernel']):
        with pytest.raises(SystemExit):
            driver.parse_args(bad)
        assert '--native_kernel' in capsys.readouterr().err
