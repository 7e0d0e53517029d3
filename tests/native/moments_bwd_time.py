"""The fused backward of the moments (ops.gram_moments_bwd, csrc/moments.hip) against a composed chunked backward built from the
ops the library had before it: per tile of 8192 points, ops.rbf_gram on the slice of X, gK = (S K + gc (w y)^T) o w by torch
products, and the gram op's own backward (K.backward(gK)), gradients accumulated over the tiles.  Shapes (G, Mt, N, D):
(1, 512, 1e5, 8) and (10, 100, 6e4, 784), RBF, unit weights.  Timed alternately with device events (median and minimum of REPS
calls after a warm-up).  The composed route stores each tile of K and of gK (2 x G x Mt x 8192 floats); the fused call stores
neither.  Also reports the relative L2 difference of the two gZ.  Feeds the collapsed section of DESIGN.md.  GPU box only."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from vargp_amd import ops  # noqa: E402

dev = torch.device('cuda', 0)
WARM, REPS, TILE = 2, 7, 8192


def composed(theta, Z, X, y, gPhi, gc):
    th = theta.view(1, -1).clone().requires_grad_(True)
    Zr = Z.clone().requires_grad_(True)
    S = gPhi + gPhi.mT
    for i in range(0, X.shape[0], TILE):
        K = ops.rbf_gram(th, Zr, X[i:i + TILE], True)                              # (1, G, Mt, tile)
        with torch.no_grad():
            gK = S @ K[0] + gc.unsqueeze(-1) * y[:, i:i + TILE].unsqueeze(-2)
        K.backward(gK.unsqueeze(0))
    return Zr.grad, th.grad.view(-1)


def timed(fn):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    out = fn()
    e[1].record()
    e[1].synchronize()
    return e[0].elapsed_time(e[1]), out


for G, Mt, N, D in ((1, 512, 100_000, 8), (10, 100, 60_000, 784)):
    g = torch.Generator(device=dev).manual_seed(0)
    scale = 1.0 if D <= 8 else 0.12
    X = scale * torch.randn(N, D, device=dev, generator=g)
    Z = torch.stack([X[torch.randperm(N, device=dev, generator=g)[:Mt]] for _ in range(G)]).contiguous()
    y = torch.randn(G, N, device=dev, generator=g)
    gPhi = torch.randn(G, Mt, Mt, device=dev, generator=g)
    gc = torch.randn(G, Mt, device=dev, generator=g)
    theta = torch.cat([torch.full((D,), math.log(0.8 * math.sqrt(D) * scale)), torch.tensor([0.0])]).to(dev)
    fns = {'fused': lambda: ops.gram_moments_bwd(theta, Z, X, None, y, gPhi, gc, 0), 'composed': lambda: composed(theta, Z, X, y, gPhi, gc)}
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    t, outs = {name: [] for name in fns}, {}
    for _ in range(REPS):
        for name, fn in fns.items():
            ms, outs[name] = timed(fn)
            t[name].append(ms)
    res = dict(G=G, Mt=Mt, N=N, D=D, tile=TILE, reps=REPS, chunks=ops.gram_moments_bwd_chunks(G, Mt, N, D),
               workspace_bytes=int(ops.lib().vargp_gram_moments_bwd_workspace_bytes(G, Mt, N, D)),
               composed_tile_bytes=2 * 4 * G * Mt * TILE,
               gZ_rel_l2_diff=((outs['fused'][0] - outs['composed'][0]).norm() / outs['composed'][0].norm()).item(),
               gtheta_rel_l2_diff=((outs['fused'][1][:D] - outs['composed'][1][:D]).norm() / outs['composed'][1][:D].norm()).item())
    for name, v in t.items():
        res[f'{name}_ms_median'], res[f'{name}_ms_min'] = statistics.median(v), min(v)
    res['composed_over_fused_median'] = res['composed_ms_median'] / res['fused_ms_median']
    print(json.dumps(res), flush=True)
    del X, Z, y
