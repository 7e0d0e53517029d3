"""ops.gram_moments (csrc/moments.hip) at N = 1e6 points -- (D, Mt) = (8, 100), (8, 500), (784, 100), one output, RBF -- against the
route the library had before it: ops.rbf_gram on tiles of 8192 points and ops.bgemm K K^T (and K y) per tile, accumulated in place.
Timed alternately with device events (median and minimum of REPS calls after a warm-up).  The composed route stores each tile of
K (Mt x 8192 floats); the fused call stores none of it.  Also reports the largest entry-wise difference of the two Phi relative to
the largest entry.  Feeds the collapsed section of DESIGN.md.  GPU box only."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from vargp_amd import ops  # noqa: E402

dev = torch.device('cuda', 0)
WARM, REPS = 2, 7
N, TILE = 1_000_000, 8192


def composed(theta, Z, X, y):
    """Phi, c tile by tile from the gram op and the batched GEMM"""
    Mt = Z.shape[1]
    Phi = torch.zeros(1, 1, Mt, Mt, device=dev)
    c = torch.zeros(1, 1, Mt, 1, device=dev)
    th = theta.view(1, -1)
    for i in range(0, X.shape[0], TILE):
        K = ops.rbf_gram(th, Z, X[i:i + TILE], True)                       # (1, 1, Mt, tile)
        ops.bgemm(K, K.mT, D=Phi, beta=1.0, out=Phi)
        ops.bgemm(K, y[:, i:i + TILE].reshape(1, 1, -1, 1), D=c, beta=1.0, out=c)
    return Phi[0], c[0, :, :, 0]


def timed(fn):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    out = fn()
    e[1].record()
    e[1].synchronize()
    return e[0].elapsed_time(e[1]), out


for D, Mt in ((8, 100), (8, 500), (784, 100)):
    g = torch.Generator(device=dev).manual_seed(0)
    X = torch.randn(N, D, device=dev, generator=g)
    Z = X[torch.randperm(N, device=dev, generator=g)[:Mt]].unsqueeze(0).contiguous()
    y = torch.randn(1, N, device=dev, generator=g)
    theta = torch.cat([torch.full((D,), math.log(0.8 * math.sqrt(D))), torch.tensor([0.0])]).to(dev)
    fns = {'gram_moments': lambda: ops.gram_moments(theta, Z, X, None, y, 0)[:2], 'composed': lambda: composed(theta, Z, X, y)}
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t, outs = {name: [] for name in fns}, {}
    for _ in range(REPS):
        for name, fn in fns.items():
            ms, outs[name] = timed(fn)
            t[name].append(ms)
    res = dict(N=N, D=D, Mt=Mt, tile=TILE, reps=REPS, chunks=ops.gram_moments_chunks(1, Mt, N, D),
               workspace_bytes=int(ops.lib().vargp_gram_moments_workspace_bytes(1, Mt, N, D)), composed_K_tile_bytes=4 * Mt * TILE,
               phi_max_rel_diff=((outs['gram_moments'][0] - outs['composed'][0]).abs().max() / outs['composed'][0].abs().max()).item())
    for name, v in t.items():
        res[f'{name}_ms_median'], res[f'{name}_ms_min'] = statistics.median(v), min(v)
    res['composed_over_fused_median'] = res['composed_ms_median'] / res['gram_moments_ms_median']
    print(json.dumps(res), flush=True)
    del X, Z, y
