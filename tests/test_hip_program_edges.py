"""GPU: both native ELBO programs at the likelihood edges the random sweeps never draw -- C > 16 (the generic softmax backward of
csrc/elbo_ops.hip instead of the fused one: its seed, scale and the programs' handling of gmu / gvar) and F > 16 (beyond the
deferred softmax of the first-task backward, F <= 4 kBmSmF) -- held to the sweep rule (tests/sweep_rule.py), and the tiled
ELBO's refusal of more than 16 classes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vargp_oracle as orc                      # noqa: E402
from sweep_rule import COST_CAP, DEV, _cost, _sweep          # noqa: E402


def _case(S, F, C, M, n_prev, D, B, seed, nomean=False, block=False):
    return dict(S=S, F=F, C=C, M=M, n_prev=n_prev, D=D, B=B, nomean=nomean, seed=seed, block=block)


# block: the case runs on the block program (csrc/elbo_tn.hip) -- every case with earlier tasks, and first tasks with M > 104
EDGE_CASES = [
    # first task, T0 program (M <= 104)
    _case(2, 16, 17, 20, 0, 8, 65, 701),
    _case(1, 17, 16, 52, 0, 40, 130, 702),
    _case(2, 20, 20, 100, 0, 4, 37, 703),
    _case(1, 16, 33, 77, 0, 784, 68, 704),
    _case(3, 17, 16, 36, 0, 33, 200, 705),
    _case(1, 16, 16, 100, 0, 40, 64, 706),
    # first task as the one-block case of the block program (M > 104)
    _case(1, 17, 17, 108, 0, 8, 65, 707, block=True),
    _case(2, 16, 20, 120, 0, 40, 30, 708, block=True),
    # one and two earlier tasks
    _case(1, 16, 17, 60, 1, 40, 65, 709, block=True),
    _case(2, 20, 33, 30, 2, 8, 36, 710, block=True),
    _case(1, 17, 16, 100, 1, 4, 128, 711, block=True),
    _case(1, 16, 20, 104, 2, 40, 70, 712, block=True),
    _case(2, 16, 17, 36, 1, 33, 68, 713, nomean=True, block=True),
    _case(1, 20, 16, 120, 1, 2, 65, 714, block=True),
]


def test_programs_at_likelihood_edges():
    """C in {16, 17, 20, 33} and F in {16, 17, 20} on the first-task program, the one-block case and one to two earlier tasks
    (ragged B, M on both sides of 100) under the sweep rule; each case on the program it is meant for."""
    for c in EDGE_CASES:
        assert _cost(c['S'], c['C'], c['M'], c['n_prev'], c['D'], c['B']) <= COST_CAP, c
    rows = _sweep(EDGE_CASES, 'likelihood edges')
    assert [r[2] for r in rows] == [c['block'] for c in EDGE_CASES]
    assert {c['C'] for c in EDGE_CASES} >= {16, 17, 20, 33} and {c['F'] for c in EDGE_CASES} >= {16, 17, 20}


def test_tiled_elbo_refuses_more_than_16_classes():
    from gpu_common import build_gp
    from vargp_amd._lib import VargpHipError
    S, F_, C, M, D, N = 1, 2, 17, 24, 40, 100
    params, prev, x, y, nz = orc.make_problem(S, F_, C, M, D, N, n_prev=1, seed=715, kind='gauss')
    gp = build_gp(params, prev, S, F_)
    with pytest.raises(VargpHipError, match='more than 16 classes'):
        gp.elbo_tiled(x.to(DEV), y.to(DEV), 64, noise_seed=3)
    torch.cuda.synchronize()
    # 16 classes are served
    params, prev, x, y, nz = orc.make_problem(S, F_, 16, M, D, N, n_prev=1, seed=716, kind='gauss')
    gp = build_gp(params, prev, S, F_)
    out = gp.elbo_tiled(x.to(DEV), y.to(DEV), 64, noise_seed=3)
    assert all(torch.isfinite(v).item() for v in out)
