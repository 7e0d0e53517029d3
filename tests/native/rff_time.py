"""ops.rff_paths (csrc/rff.hip: the random Fourier features never leave the chip) against the composition of existing ops it
replaces -- the frequencies pre-scaled by the lengthscales, ops.bgemm for the phases, torch.cos / torch.sin and the
gamma / sqrt(R) scale, ops.bgemm with the weights -- at S C = 30, D = 784, R = 1024, N = 8: x_shared = 1 with n = 4096 (a block of
test points) and x_shared = 0 with n = 200 (the inducing points).  The two are timed alternately with device events (median and
minimum of REPS calls after a warm-up) and their results compared.  Feeds the pathwise-samples section of DESIGN.md.  GPU box
only."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from vargp_amd import ops  # noqa: E402

dev = torch.device('cuda', 0)
S, C, D, R, N = 3, 10, 784, 1024, 8
WARM, REPS = 3, 15
g = torch.Generator(device=dev).manual_seed(0)
theta = math.log(2.5) + 0.05 * torch.randn(S, D + 1, device=dev, generator=g)
theta[:, -1] = math.log(0.5)
omega = torch.randn(R, D, device=dev, generator=g)
coef = torch.randn(S, C, 2 * R, N, device=dev, generator=g)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


for shared, n in ((True, 4096), (False, 200)):
    shape = (n, D) if shared else (C, n, D)
    x = torch.rand(*shape, device=dev, generator=g) * (torch.rand(*shape, device=dev, generator=g) < 0.19)      # MNIST-like pixels

    def fused():
        return ops.rff_paths(theta, x, omega, coef, shared)

    def composed():
        om = omega.unsqueeze(0) * (-theta[:, :-1]).exp().unsqueeze(1)                        # (S, R, D)
        p = ops.bgemm(x, om.mT) if shared else ops.bgemm(x.unsqueeze(0), om.mT.unsqueeze(1))  # (S, n, R) | (S, C, n, R)
        Phi = torch.cat([p.cos(), p.sin()], dim=-1) * (theta[:, -1].exp() / math.sqrt(R)).view(S, *([1] * (p.dim() - 1)))
        return ops.bgemm(Phi.unsqueeze(1) if shared else Phi, coef)                           # (S, C, n, N)

    for _ in range(WARM):
        fused(), composed()
    torch.cuda.synchronize()
    tf, tc = [], []
    for _ in range(REPS):
        t, a = timed(fused)
        tf.append(t)
        t, b = timed(composed)
        tc.append(t)
    diff = (a - b).abs().max().item()
    assert a.shape == b.shape == (S, C, n, N)
    assert diff <= 1e-3 * 0.5, diff                           # gamma = 0.5: the two agree to the fp32 rounding of the phases
    nset = S if shared else S * C
    flop = 2.0 * nset * n * R * D + 2.0 * S * C * n * 2 * R * N
    feat_bytes = 4.0 * nset * n * 2 * R                       # the feature matrix the composition writes and reads back
    print(json.dumps(dict(x_shared=int(shared), S=S, C=C, n=n, D=D, R=R, N=N, reps=REPS,
                          fused_ms_median=statistics.median(tf), fused_ms_min=min(tf),
                          composed_ms_median=statistics.median(tc), composed_ms_min=min(tc),
                          speedup_median=statistics.median(tc) / statistics.median(tf),
                          max_abs_diff=diff, gamma=0.5, gflop=flop / 1e9,
                          feature_matrix_mb=feat_bytes / 1e6)), flush=True)
