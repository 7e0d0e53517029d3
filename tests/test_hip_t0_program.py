"""GPU: the native first-task ELBO program (vargp_elbo_t0_fwd / _bwd) against the fp64 oracle on shapes that hit
its edge paths, and the trainer's direct use of it against the autograd route.  (tests/test_t0_plan.py asserts, without a
GPU, that every shape of SHAPES takes the path its comment names on 256 CUs.)"""
import numpy as np
import pytest
import torch

from oracle import vargp_oracle as orc
from helpers import rel_l2, to_dev, RTOL_SCALAR, REL_L2_GRAD

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _problem(S, F_, C, M, D, B, seed, kind='gauss'):
    params, prev, x, y, nz = orc.make_problem(S, F_, C, M, D, B, n_prev=0, seed=seed, kind=kind)
    return params, prev, x, y, nz


# (S, F, C, M, D, B): odd M (padded small-column block), B not a multiple of 4 (padded row stride, scalar GEMM
# loads), C > 16 (generic softmax kernels), D <= 32 (direct distance form), M > 100 (blocked Cholesky)
SHAPES = [(2, 3, 3, 33, 40, 50), (3, 2, 4, 20, 64, 37), (2, 2, 18, 12, 36, 24), (2, 3, 2, 20, 2, 64),
          (1, 2, 2, 130, 48, 40),
          # tiny / degenerate: one class, one hyper-sample, one likelihood sample, 3 inducing points, 2 data points;
          # M = 64 and M = 65 (the two register-slot layouts of the factorisation kernel), M = 100 with B % 4 != 0
          (1, 1, 1, 3, 33, 2), (2, 2, 2, 64, 40, 33), (2, 2, 2, 65, 40, 32), (1, 2, 2, 100, 36, 50), (1, 2, 3, 51, 36, 8),
          # the LDS-resident backward (t0_bwd_mid.h / t0_bwd_mat.h: M % 4 == 0, M <= 104, B % 4 == 0, D % 4 == 0): ragged last
          # 64-column tile, M = 104 (no padding left), M = 4, four / five / eight / sixteen / seventeen hyper-samples (the S_u chains
          # redo S products; more than four: the tail's operands staged through LDS), several full tiles
          (3, 2, 3, 100, 40, 72), (4, 2, 2, 104, 36, 64), (5, 2, 2, 52, 36, 40), (2, 2, 2, 4, 36, 8), (2, 3, 3, 96, 48, 200),
          (3, 2, 2, 100, 36, 132), (8, 2, 2, 100, 36, 64), (16, 1, 2, 100, 36, 64), (17, 2, 2, 52, 36, 40),
          # the persistent P_uf role of the backward's merged launch (gemm_persist_body: more tiles than free CUs, B % 64 == 0,
          # B >= 256): static tile lists with four (the minimum) and five slabs per tile, and the work queue that the finished
          # matrix chains join (more than four tiles per free CU: 7 x 16 x 7 = 784 tiles for 256 - 80 CUs; seven hyper-samples keep
          # the S C + C = 80 chains below the third of the CU count from which the launches are taken apart)
          (3, 2, 10, 100, 784, 256), (3, 2, 10, 100, 784, 320), (7, 2, 10, 100, 448, 256),
          # more (s, c, tile) units than CUs: the multi-tile form of the LDS-resident tile kernels (a workgroup walks several tiles
          # of its (s, c): T / G staged once, M x M accumulators kept across tiles) -- uneven tile shares (8 tiles over 3
          # workgroups), a ragged last tile, B % 4 != 0 (the per-element K_uf loads), and one workgroup for all tiles of a matrix
          (8, 2, 10, 100, 36, 512), (6, 2, 10, 96, 36, 328), (12, 1, 9, 100, 36, 200), (10, 2, 10, 52, 36, 130),
          (16, 1, 16, 100, 36, 128),
          # many per-matrix chains (S C + C > a third of the CUs): the role-merged launches taken apart -- chains alone on a side stream,
          # K_uf / P_uf as launches of their own, the S_u roles of the backward reading the per-class sums of the L_S gradient shares
          # that the K_uu roles accumulate (BwdMatArgs::gL_acc); 17 and 33 hyper-samples
          (17, 1, 16, 52, 36, 64), (33, 1, 8, 100, 36, 72),
          # ... D >= 256: behind the front launch (x o w operand), the Gram matrices built by the chain workgroups (chol_gram.h)
          (13, 1, 10, 100, 256, 128),
          # the tile kernels WITHOUT the per-matrix chains / fused tail (T0Plan: fused_bwd but not mat_bwd): D % 4 != 0, and
          # more hyper-samples than the tail kernels take (S > kTailSMax = 64)
          (3, 2, 2, 52, 38, 40), (65, 1, 2, 52, 36, 40)]


@pytest.mark.parametrize('shape', SHAPES, ids=[str(s) for s in SHAPES])
def test_program_matches_fp64_oracle(shape):
    from vargp_amd import noise
    from gpu_common import build_gp, grads_of
    S, F_, C, M, D, B = shape
    params, prev, x, y, nz = _problem(S, F_, C, M, D, B, seed=31)
    gp = build_gp(params, prev, S, F_)
    with noise.inject(**to_dev(nz, DEV)):
        kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
        (2.0 * kl_h + kl_u + 7.0 * nll).backward()
    sc, og = orc.elbo_step(params, prev, x, y, nz, beta=2.0, n_total=7 * B)
    for k, v in [('kl_hypers', kl_h), ('kl_u', kl_u), ('nll', nll)]:
        np.testing.assert_allclose(v.item(), sc[k].item(), rtol=RTOL_SCALAR, err_msg=k)
    # D = 2 with 20 inducing points per class: K_uu + 1e-4 I has a condition number ~1e5, which amplifies the fp32 rounding of
    # the factorisation into the hyper-parameter gradients (measured over 2000 repeats: log_logvar 1.01e-3 .. 1.05e-3 against
    # the fp64 oracle, moving with the order of the float atomics; every other shape stays below 3e-4)
    tol = 2 * REL_L2_GRAD if D <= 2 else REL_L2_GRAD
    for k, g in grads_of(gp).items():
        assert rel_l2(g.cpu(), og[k]) < tol, k


def _random_shapes(n, seed):
    """Shapes drawn inside and around the limits of the LDS-resident kernels (tests/native/t0_random_sweep.py runs more)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        out.append((int(rng.integers(1, 10)), int(rng.integers(1, 4)), int(rng.integers(1, 13)),
                    int(rng.choice([4, 8, 12, 20, 32, 36, 52, 60, 64, 68, 96, 100, 104, 23, 51, 77, 108])),
                    int(rng.choice([8, 36, 40, 64, 100, 260, 300, 33, 37])),
                    int(rng.choice([4, 8, 36, 60, 64, 68, 128, 132, 200, 30, 65]))))
    return out


RANDOM_SHAPES = _random_shapes(14, 7)


@pytest.mark.parametrize('shape', RANDOM_SHAPES, ids=[str(s) for s in RANDOM_SHAPES])
def test_program_random_shapes_vs_fp64_oracle(shape):
    from vargp_amd import noise
    from gpu_common import build_gp, grads_of
    S, F_, C, M, D, B = shape
    params, prev, x, y, nz = _problem(S, F_, C, M, D, B, seed=77)
    gp = build_gp(params, prev, S, F_)
    with noise.inject(**to_dev(nz, DEV)):
        kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
        (2.0 * kl_h + kl_u + 7.0 * nll).backward()
    sc, og = orc.elbo_step(params, prev, x, y, nz, beta=2.0, n_total=7 * B)
    for k, v in [('kl_hypers', kl_h), ('kl_u', kl_u), ('nll', nll)]:
        np.testing.assert_allclose(v.item(), sc[k].item(), rtol=RTOL_SCALAR, err_msg=k)
    for k, g in grads_of(gp).items():
        assert rel_l2(g.cpu(), og[k]) < REL_L2_GRAD, k


def test_program_map_est():
    """map_est: theta = log_mean, no hyper-KL; against the composed per-op path."""
    from vargp_amd import noise
    from gpu_common import build_gp, grads_of
    S, F_, C, M, D, B = 1, 3, 3, 24, 40, 32
    params, prev, x, y, nz = _problem(S, F_, C, M, D, B, seed=5)
    res = []
    for fused in (True, False):
        gp = build_gp(params, prev, S, F_)
        gp.kernel.map_est = True
        gp.fused_first_task = fused
        with noise.inject(eps_f=nz['eps_f'].to(DEV)):
            kl_h, kl_u, nll = gp.loss(x.to(DEV), y.to(DEV))
            (kl_h + kl_u + 3.0 * nll).backward()
        g = grads_of(gp)
        assert g['log_logvar'] is None
        res.append(((kl_h.item(), kl_u.item(), nll.item()), {k: v.cpu() for k, v in g.items() if v is not None}))
    assert res[0][0][0] == 0.0
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-5)
    for k in res[1][1]:
        assert rel_l2(res[0][1][k], res[1][1][k]) < 1e-4, k


def test_trainer_direct_program_equals_autograd_route():
    """ElboTrainer drives T0Program directly (seeds, gradients written into the optimiser's buffers); the same
    steps through gp.loss -> autograd -> Yogi must give the same parameters."""
    import vargp_amd
    from vargp_amd import noise
    from vargp_amd.optim import Yogi
    from vargp_amd.train import ElboTrainer
    from gpu_common import build_gp
    S, F_, C, M, D, B = 2, 3, 4, 30, 48, 64
    params, prev, x, y, nz = _problem(S, F_, C, M, D, B, seed=8, kind='mnist')
    xd, yd = x.to(DEV), y.to(DEV)
    beta, n_total = 1.5, 10 * B
    gp_a, gp_b = build_gp(params, prev, S, F_), build_gp(params, prev, S, F_)
    tr = ElboTrainer(gp_a, lr=3e-3, beta=beta, n_total=n_total)
    assert tr._t0
    opt = Yogi([p for p in gp_b.parameters() if p.requires_grad], lr=3e-3)
    for it in range(3):
        nzd = {k: (v + 0.1 * it).to(DEV) for k, v in nz.items()}
        with noise.inject(**nzd):
            out_a = [float(v) for v in tr.step(xd, yd)]
            for p in gp_b.parameters():
                p.grad = None
            kl_h, kl_u, nll = gp_b.loss(xd, yd)
            (beta * kl_h + kl_u + (n_total / B) * nll).backward()
            opt.step()
        np.testing.assert_allclose(out_a, [kl_h.item(), kl_u.item(), nll.item()], rtol=1e-5)
    for (k, pa), (_, pb) in zip(gp_a.named_parameters(), gp_b.named_parameters()):
        assert rel_l2(pa.detach().cpu(), pb.detach().cpu()) < 1e-5, k


def test_program_rejects_bad_arguments():
    from vargp_amd._lib import VargpHipError
    from vargp_amd.fused import T0Program
    prog = T0Program(1, 2, 8, 4, 8, 2, DEV, map_est=False)
    z = torch.zeros(2, 8, 4, device=DEV)
    with pytest.raises(VargpHipError):        # CPU tensor: no CPU path
        prog.forward(torch.zeros(5), torch.zeros(5), torch.zeros(5), torch.zeros(5), z, z[..., :1], z[..., :1],
                     torch.zeros(8, 4), torch.zeros(8, dtype=torch.int64), torch.zeros(1, 5), torch.zeros(1, 2, 2, 8))
    with pytest.raises(RuntimeError, match='one backward per forward'):       # backward before forward
        prog.backward(*([torch.zeros(3, device=DEV)] * 6))


def test_c_abi_enforces_one_backward_per_forward():
    """include/vargp_hip.h: on the LDS-resident backward path the forward clears the accumulators the backward adds into; the
    library itself (not only the Python wrapper) refuses a second vargp_elbo_t0_bwd on one forward."""
    import ctypes
    from vargp_amd import noise
    from vargp_amd._lib import VargpHipError, check, lib, ptr, stream_ptr
    from vargp_amd.fused import T0Program
    S, F_, C, M, D, B = 2, 3, 3, 56, 40, 64                 # M <= 104, M % 4 == 0, B % 4 == 0, D % 4 == 0: that path
    params, prev, x, y, nz = orc.make_problem(S, F_, C, M, D, B, seed=5, kind='gauss')
    p = {k: v.to(DEV).contiguous() for k, v in params.items()}
    prog = T0Program(S, C, M, D, B, F_, DEV)
    seeds = torch.ones(3, device=DEV)
    grads = [torch.empty_like(p[k]) for k in ('log_mean', 'log_logvar', 'z', 'u_mean', 'u_tril_vec')]
    args = (p['log_mean'], p['log_logvar'], p['prior_log_mean'], p['prior_log_logvar'], p['z'], p['u_mean'], p['u_tril_vec'],
            x.to(DEV), y.to(DEV), nz['eps_theta'].to(DEV), nz['eps_f'].to(DEV))
    prog.forward(*args)
    prog.backward(seeds, *grads)
    g1 = [g.clone() for g in grads]
    call = lambda: check(lib().vargp_elbo_t0_bwd(ctypes.byref(prog.desc), ptr(seeds), *(ptr(g) for g in grads), stream_ptr()),
                         'vargp_elbo_t0_bwd')
    with pytest.raises(VargpHipError, match='ONE vargp_elbo_t0_bwd per vargp_elbo_t0_fwd'):
        call()                                            # straight through the C ABI, past the wrapper's own check
    prog.forward(*args)                                   # a new forward re-arms it, and the result is the same
    call()
    for a, b in zip(grads, g1):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5)
