"""vargp_rff_paths_bwd (csrc/rff.hip: the gradient of the random-Fourier-feature paths in their points, neither phases, features
nor h stored) against the composition of existing ops it replaces -- the frequencies pre-scaled by the lengthscales, ops.bgemm for
the phases, torch.sin / torch.cos, ops.bgemm for gout coef^T (cos rows and sin rows), the elementwise combination into h (stored),
ops.bgemm for h om and the sum over the hyper-samples -- at S = 3, C = 10, n = 512, D = 784, R = 1024, N = 4, x_shared = 1.  The
fused entry is timed at its launch site (vargp_prof_enable / vargp_prof_read, tag rff_paths_bwd: the pre-scaling launch, the fused
kernel and the reduction of the partial sums); both routes are also timed alternately with device events (median and minimum of
REPS calls after a warm-up) and their results compared.  Feeds the differentiable-paths section of DESIGN.md.  GPU box only."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from vargp_amd import _lib, ops  # noqa: E402

dev = torch.device('cuda', 0)
S, C, n, D, R, N = 3, 10, 512, 784, 1024, 4
WARM, REPS = 5, 30
g = torch.Generator(device=dev).manual_seed(0)
theta = math.log(2.5) + 0.05 * torch.randn(S, D + 1, device=dev, generator=g)
theta[:, -1] = math.log(0.5)
omega = torch.randn(R, D, device=dev, generator=g)
coef = torch.randn(S, C, 2 * R, N, device=dev, generator=g)
gout = torch.randn(S, C, n, N, device=dev, generator=g)
x = torch.rand(n, D, device=dev, generator=g) * (torch.rand(n, D, device=dev, generator=g) < 0.19)             # MNIST-like pixels
xg = x.clone().requires_grad_(True)
out = ops.rff_paths_x(theta, xg, omega, coef, True)                                    # the graph, once


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    res = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), res


def fused():
    return torch.autograd.grad(out, xg, gout, retain_graph=True)[0]


def composed():
    om = omega.unsqueeze(0) * (-theta[:, :-1]).exp().unsqueeze(1)                             # (S, R, D)
    p = ops.bgemm(x, om.mT)                                                                   # (S, n, R)
    G = gout.permute(0, 2, 1, 3).reshape(S, n, C * N)                                         # (S, n, C N)
    W = coef.permute(0, 2, 1, 3).reshape(S, 2 * R, C * N)                                     # (S, 2R, C N)
    T = ops.bgemm(G, W.mT)                                                                    # (S, n, 2R)
    h = (T[..., R:] * p.cos() - T[..., :R] * p.sin()) * (theta[:, -1].exp() / math.sqrt(R)).view(S, 1, 1)
    return ops.bgemm(h, om).sum(0)                                                            # (n, D)


for _ in range(WARM):
    fused(), composed()
torch.cuda.synchronize()
tf, tc = [], []
for _ in range(REPS):
    t, a = timed(fused)
    tf.append(t)
    t, b = timed(composed)
    tc.append(t)
scale = b.abs().max().item()
diff = (a - b).abs().max().item() / scale
assert a.shape == b.shape == (n, D)
assert diff <= 1e-3, diff                                     # the two agree to the fp32 rounding of the phases
_lib.prof_enable(True)
for _ in range(REPS):
    fused()
torch.cuda.synchronize()
ms, cnt = _lib.prof_read('rff_paths_bwd')
_lib.prof_enable(False)
flop = 2.0 * S * n * R * D * 2 + 2.0 * S * n * 2 * R * C * N
print(json.dumps(dict(S=S, C=C, n=n, D=D, R=R, N=N, x_shared=1, reps=REPS,
                      fused_prof_ms=ms / max(cnt, 1), prof_launches=cnt,
                      fused_ms_median=statistics.median(tf), fused_ms_min=min(tf),
                      composed_ms_median=statistics.median(tc), composed_ms_min=min(tc),
                      speedup_median=statistics.median(tc) / statistics.median(tf),
                      max_rel_diff=diff, gflop=flop / 1e9, stored_by_the_composition_mb=4.0 * S * n * 5 * R / 1e6)), flush=True)
