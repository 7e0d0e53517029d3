"""ops.predictive_cov (csrc/pred_cov.hip: one pass over the S C B^2 covariance) against the composition of existing ops it
replaces -- rbf_gram(theta, x), then two bgemm calls accumulating in place (-P^T P + K, then + W^T W) -- at S C = 30, B = 1024,
D = 784, Mt = 200 and 1000.  The two are timed alternately with device events (median and minimum of REPS calls after a warm-up)
and their results compared.  Feeds the predictive-covariance section of DESIGN.md.  GPU box only."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from vargp_amd import ops  # noqa: E402

dev = torch.device('cuda', 0)
S, C, B, D = 3, 10, 1024, 784
WARM, REPS = 3, 15
g = torch.Generator(device=dev).manual_seed(0)
theta = math.log(2.5) + 0.05 * torch.randn(S, D + 1, device=dev, generator=g)
theta[:, -1] = math.log(0.5)
x = torch.rand(B, D, device=dev, generator=g) * (torch.rand(B, D, device=dev, generator=g) < 0.19)      # MNIST-like pixels


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


for Mt in (200, 1000):
    P = 0.5 * torch.randn(S, C, Mt, B, device=dev, generator=g) / math.sqrt(Mt)
    W = 0.5 * torch.randn(S, C, Mt, B, device=dev, generator=g) / math.sqrt(Mt)

    def fused():
        return ops.predictive_cov(theta, x, P, W, 0)

    def composed():
        K = ops.rbf_gram(theta, x.unsqueeze(0))                                  # (S, 1, B, B)
        out = ops.bgemm(P.mT, P, alpha=-1.0, D=K, beta=1.0)                      # (S, C, B, B)
        return ops.bgemm(W.mT, W, alpha=1.0, D=out, beta=1.0, out=out)

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
    flop = 2.0 * S * C * B * B * (D + 2 * Mt)            # the full square; the fused kernel computes the lower tiles only
    print(json.dumps(dict(S=S, C=C, B=B, D=D, Mt=Mt, reps=REPS,
                          fused_ms_median=statistics.median(tf), fused_ms_min=min(tf),
                          composed_ms_median=statistics.median(tc), composed_ms_min=min(tc),
                          speedup_median=statistics.median(tc) / statistics.median(tf),
                          max_abs_diff=diff, gamma2=0.25, full_square_gflop=flop / 1e9)), flush=True)
