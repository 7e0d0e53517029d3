"""torch.autograd.Function wrappers over the C ABI: every forward AND backward below is a call into
libvargp_hip.so (hand-written HIP), torch only owns the memory and the stream.
"""
import math
from collections import namedtuple

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import GemmDesc, check, lib, ptr, require_device, scratch, stream_ptr

NONE, LOWER, UPPER = 0, 1, 2
_FLIP = {NONE: NONE, LOWER: UPPER, UPPER: LOWER}
JITTER = 1e-4

# Cholesky failures: 'raise' syncs after every factorisation (what torch.cholesky does, reference
# var_gp/gp_utils.py:10); 'defer' never syncs (hipGraph-capturable): failed factors are NaN-filled and
# the flag is accumulated on device, readable with linalg_error_count().
_chol_mode = 'raise'
_info_ring = []   # 'defer' mode: most recent info tensors (device), inspected on demand


_lazy_rings = {}
_pending = []     # 'lazy' mode: (pinned host copy of an info tensor, event recorded behind the copy)


def set_cholesky_error_mode(mode):
    """What happens when a factorisation meets a matrix that is not positive definite (the reference's torch.cholesky raises,
    gp_utils.py:5-11 -- which costs it a device synchronisation per call):
      'raise'  (default) the same: every factorising call waits for its status words and raises torch.linalg.LinAlgError;
      'lazy'   no wait: the status words are copied to pinned host memory behind the call, and the error is raised by the NEXT
               factorising call, by the first host read of one of the step's values (ElboTerm.item() / float()), or by
               check_linalg_errors() -- at most one step late, never lost;
      'defer'  nothing is read back until linalg_error_count() is asked for (captured hipGraphs: no host work inside a step)."""
    global _chol_mode
    assert mode in ('raise', 'lazy', 'defer')
    check_linalg_errors()
    _chol_mode = mode


def check_linalg_errors(wait=False):
    """'lazy' mode: raise for any failed factorisation whose status words have arrived (wait: all of them, synchronising)."""
    bad = None
    while _pending:
        host, ev = _pending[0]
        if wait:
            ev.synchronize()
        elif not ev.query():
            break
        _pending.pop(0)
        n = int((host != 0).sum())
        if n and bad is None:
            bad = (n, host.numel(), int(host[host != 0][0]))
    if bad is not None:
        del _pending[:]
        raise torch.linalg.LinAlgError(f'vargp_chol_inv: {bad[0]} of {bad[1]} matrices are not positive-definite '
                                       f'(first failing leading minor of order {bad[2]}; reported lazily)')


def reset_linalg_errors():
    del _info_ring[:]


def linalg_error_count_begin():
    """'defer' mode, for callers that synchronise anyway (the driver's one sync per epoch): ENQUEUE the count of failed
    factorisations and its copy to pinned memory on the current stream -> a handle; `int(handle)` after the caller's own
    synchronisation is the count.  (linalg_error_count() after a sync starts its reductions on an idle GPU and waits for them:
    ~0.1 ms per epoch that this form hides in the pipeline.)"""
    uniq = {}
    for t in _info_ring:
        uniq[(t.data_ptr(), t.numel())] = t
    slot = _lazy_rings.get('count')
    if slot is None:
        slot = _lazy_rings['count'] = torch.zeros(1, dtype=torch.int64, pin_memory=True)
    if not uniq:
        slot.zero_()
        return slot
    counts = [torch.count_nonzero(t) for t in uniq.values()]
    total = torch.stack(counts).sum() if len(counts) > 1 else counts[0]
    slot.copy_(total.view(1), non_blocking=True)
    return slot


def linalg_error_count():
    """'defer' mode: number of failed factorisations among the most recent calls.  ONE host sync: the ring usually holds the
    same few info tensors many times over (a program's info buffer is appended on every eager call), so they are counted
    once each, and the counts are summed on the device before the single read-back."""
    uniq = {}
    for t in _info_ring:
        uniq[(t.data_ptr(), t.numel())] = t
    if not uniq:
        return 0
    counts = [torch.count_nonzero(t) for t in uniq.values()]
    return int(torch.stack(counts).sum().item()) if len(counts) > 1 else int(counts[0].item())


# ------------------------------------------------------------------------------------------------
# low-level batched GEMM (no autograd)
# ------------------------------------------------------------------------------------------------
def _mat_layout(t):
    """-> (tensor, trans, ld): trans=0 if rows are contiguous (stride(-1)==1), 1 if it is a
    transposed view (stride(-2)==1); otherwise a contiguous copy is made."""
    r, c = t.shape[-2], t.shape[-1]
    s2, s1 = t.stride(-2), t.stride(-1)
    if s1 == 1 and (s2 >= c or r == 1):
        return t, 0, max(s2, c) if r > 1 else max(c, 1)
    if s2 == 1 and (s1 >= r or c == 1):
        return t, 1, max(s1, r) if c > 1 else max(r, 1)
    t = t.contiguous()
    return t, 0, max(c, 1)


def _batch3(shape, strides):
    """collapse batch dims to exactly 3 (pad in front); -> (sizes, strides) or None if > 3 dims"""
    if len(shape) > 3:
        return None
    pad = 3 - len(shape)
    return [1] * pad + list(shape), [0] * pad + list(strides)


def _gemm_desc(A, B, D, C, alpha, beta, triA, triB, triC):
    """The GemmDesc of C = alpha * A @ B + beta * D, -> (desc, keep, C): layouts, leading dimensions, the three batch sizes and
    strides (in elements) and the pointers.  `keep` = [A, B(, D)] as the descriptor addresses them -- the caller's own views
    wherever the kernel can consume them in place, contiguous copies otherwise -- and has to outlive the launch.  C = None: the
    result is allocated here.  No device check and no launch: the addressing is the same for host tensors, which is how the
    suite checks it."""
    M, K = A.shape[-2:]
    K2, N = B.shape[-2:]
    assert K == K2, (A.shape, B.shape)
    bshape = torch.broadcast_shapes(A.shape[:-2], B.shape[:-2], D.shape[:-2] if D is not None else ())
    Ae = A.expand(*bshape, M, K)
    Be = B.expand(*bshape, K, N)
    Ae, tA, lda = _mat_layout(Ae)
    Be, tB, ldb = _mat_layout(Be)
    if len(bshape) > 3:
        Ae = Ae.reshape(-1, M, K)
        Be = Be.reshape(-1, K, N)
        Ae, tA, lda = _mat_layout(Ae)
        Be, tB, ldb = _mat_layout(Be)
    if C is None:
        C = torch.empty(*bshape, M, N, dtype=torch.float32, device=A.device)
    assert tuple(C.shape) == (*bshape, M, N) and (C.stride(-1) == 1 or N == 1), 'bgemm: bad `out`'
    # (view, not reshape: where the batch dimensions of a strided `out` do not fold into one, reshape would hand back a copy,
    #  and the product would be written there)
    Cv = C.view(-1, M, N) if len(bshape) > 3 else C
    nbs, sA = _batch3(Ae.shape[:-2], Ae.stride()[:-2])
    _, sB = _batch3(Be.shape[:-2], Be.stride()[:-2])
    _, sC = _batch3(Cv.shape[:-2], Cv.stride()[:-2])
    d = GemmDesc()
    d.M, d.N, d.K = M, N, K
    d.transA, d.transB = tA, tB
    d.A, d.B, d.C = Ae.data_ptr(), Be.data_ptr(), Cv.data_ptr()
    d.lda, d.ldb, d.ldc = lda, ldb, (max(Cv.stride(-2), N) if M > 1 else max(N, 1))
    keep = [Ae, Be]
    if D is not None:
        De = D.expand(*bshape, M, N)
        # the kernel reads D[row * ldd + col] with ldd >= N: a D broadcast over columns (stride(-1) == 0) or over rows
        # (stride(-2) == 0 < N) has no such form
        if (De.stride(-1) != 1 and N > 1) or (M > 1 and De.stride(-2) < N):
            De = De.contiguous()
        if len(bshape) > 3:
            De = De.reshape(-1, M, N)
        _, sD = _batch3(De.shape[:-2], De.stride()[:-2])
        d.D, d.ldd = De.data_ptr(), max(De.stride(-2), N) if M > 1 else max(N, 1)
        keep.append(De)
    else:
        sD = [0, 0, 0]
        d.D, d.ldd = None, 0
    for i in range(3):
        d.nb[i] = nbs[i]
        d.sA[i], d.sB[i], d.sC[i], d.sD[i] = sA[i], sB[i], sC[i], sD[i]
    d.alpha, d.beta = float(alpha), float(beta)
    d.triA, d.triB, d.triC = triA, triB, triC
    return d, keep, C


def bgemm(A, B, alpha=1.0, D=None, beta=0.0, triA=NONE, triB=NONE, triC=NONE, out=None):
    """C = alpha * A @ B + beta * D on the MFMA GEMM; A: (..., M, K), B: (..., K, N) with
    broadcasting over the leading dims (views with stride 0 and .mT views are consumed in place)."""
    require_device(A, B, D)
    assert A.dtype == torch.float32 and B.dtype == torch.float32
    if A.shape[-1] == 0:
        # an empty sum: nothing to launch (and empty operands have no address to hand over); C = beta * D, or zeros
        M, N = A.shape[-2], B.shape[-1]
        bshape = torch.broadcast_shapes(A.shape[:-2], B.shape[:-2], D.shape[:-2] if D is not None else ())
        C = out if out is not None else torch.empty(*bshape, M, N, dtype=torch.float32, device=A.device)
        assert B.shape[-2] == 0 and tuple(C.shape) == (*bshape, M, N), 'bgemm: bad `out`'
        if D is not None:
            torch.mul(D.expand(*bshape, M, N), float(beta), out=C)
        else:
            C.zero_()
        return C
    d, keep, C = _gemm_desc(A, B, D, out, alpha, beta, triA, triB, triC)
    if d.M > 0 and d.N > 0 and C.numel() > 0:
        check(lib().vargp_bgemm(d, stream_ptr()), 'vargp_bgemm')
    return C


def _reduce_to(g, shape):
    """sum a broadcast gradient back to `shape` (leading-dim broadcasts go through vargp_sum_outer)."""
    if tuple(g.shape) == tuple(shape):
        return g
    lead = g.dim() - len(shape)
    # fold size-1 leading dims of `shape` into the reduction as long as everything behind them matches
    k = 0
    while k < len(shape) and shape[k] == 1 and g.shape[lead + k] != 1:
        k += 1
    if tuple(g.shape[lead + k:]) == tuple(shape[k:]):
        g = g.contiguous()
        outer = 1
        for s in g.shape[:lead + k]:
            outer *= s
        out = torch.empty(shape, dtype=g.dtype, device=g.device)
        check(lib().vargp_sum_outer(ptr(g), ptr(out), outer, out.numel(), stream_ptr()), 'vargp_sum_outer')
        return out
    # general (interior) broadcast: rare, tiny tensors
    if lead:
        g = g.sum(dim=tuple(range(lead)))
    dims = tuple(i for i, (a, b) in enumerate(zip(g.shape, shape)) if a != b)
    return g.sum(dim=dims, keepdim=True) if dims else g


class _MatMul(Function):
    @staticmethod
    def forward(ctx, A, B, D, alpha, beta, triA, triB, triC):
        ctx.save_for_backward(A, B)
        ctx.cfg = (alpha, beta, triA, triB, triC, D.shape if D is not None else None)
        return bgemm(A, B, alpha, D, beta, triA, triB, triC)

    @staticmethod
    @once_differentiable
    def backward(ctx, gC):
        A, B = ctx.saved_tensors
        alpha, beta, triA, triB, triC, dshape = ctx.cfg
        gA = gB = gD = None
        gC = gC.contiguous() if gC.stride(-1) != 1 and gC.stride(-2) != 1 else gC
        if ctx.needs_input_grad[0]:
            gA = bgemm(gC, B.mT, alpha, triB=_FLIP[triB], triC=LOWER if triA == LOWER else NONE)
            gA = _reduce_to(gA, A.shape)
        if ctx.needs_input_grad[1]:
            gB = bgemm(A.mT, gC, alpha, triA=_FLIP[triA], triC=LOWER if triB == LOWER else NONE)
            gB = _reduce_to(gB, B.shape)
        if dshape is not None and ctx.needs_input_grad[2]:
            gD = _reduce_to(gC * beta if beta != 1.0 else gC, dshape)
        return gA, gB, gD, None, None, None, None, None


def matmul(A, B, D=None, alpha=1.0, beta=1.0, triA=NONE, triB=NONE, triC=NONE):
    """alpha * A @ B (+ beta * D).  tri* are structure hints for the LOGICAL operands; triC=LOWER is
    only meaningful (and only allowed) for lower x lower products."""
    assert triC == NONE or (triA == LOWER and triB == LOWER)
    return _MatMul.apply(A, B, D, alpha, beta if D is not None else 0.0, triA, triB, triC)


# ------------------------------------------------------------------------------------------------
# RBF and Matern (nu = 1/2, 3/2, 5/2) gram
# ------------------------------------------------------------------------------------------------
_MATERN_NU2 = {0.5: 1, 1.5: 3, 2.5: 5}
_GRAM_ENTRIES = {False: ('vargp_rbf_workspace_bytes', 'vargp_rbf_gram_fwd', 'vargp_rbf_gram_bwd'),
                 True: ('vargp_matern_workspace_bytes', 'vargp_matern_gram_fwd', 'vargp_matern_gram_bwd')}


class _Gram(Function):
    """nu2 = 0: RBF; 1, 3, 5: Matern (its entries take nu2 behind y_shared)."""
    @staticmethod
    def forward(ctx, theta, X, Y, y_shared, nu2):
        require_device(theta, X, Y)
        theta, X = theta.contiguous(), X.contiguous()
        Y = Y.contiguous() if Y is not None else None
        S, C, M, D = theta.shape[0], X.shape[0], X.shape[1], X.shape[2]
        N = M if Y is None else Y.shape[-2]
        ws_bytes, fwd, _ = _GRAM_ENTRIES[nu2 != 0]
        K = torch.empty(S, C, M, N, dtype=torch.float32, device=X.device)
        ws = scratch(getattr(lib(), ws_bytes)(S, C, M, N, D, 0), X.device)
        kind = (int(y_shared), nu2) if nu2 else (int(y_shared),)
        check(getattr(lib(), fwd)(ptr(theta), ptr(X), ptr(Y), ptr(K), S, C, M, N, D, *kind, ptr(ws), ws.numel() * 4,
                                  stream_ptr()), fwd)
        ctx.save_for_backward(theta, X, Y, K)
        ctx.kind, ctx.nu2 = kind, nu2
        return K

    @staticmethod
    @once_differentiable
    def backward(ctx, gK):
        theta, X, Y, K = ctx.saved_tensors
        S, C, M, D = theta.shape[0], X.shape[0], X.shape[1], X.shape[2]
        N = M if Y is None else Y.shape[-2]
        ws_bytes, _, bwd = _GRAM_ENTRIES[ctx.nu2 != 0]
        gK = gK.contiguous()
        gX = torch.empty_like(X)
        want_gY = Y is not None and ctx.needs_input_grad[2]
        gY = torch.empty_like(Y) if want_gY else None
        gtheta = torch.empty_like(theta)
        ws = scratch(getattr(lib(), ws_bytes)(S, C, M, N, D, 1), X.device)
        check(getattr(lib(), bwd)(ptr(theta), ptr(X), ptr(Y), ptr(K), ptr(gK), ptr(gX), ptr(gY), ptr(gtheta), S, C, M, N, D,
                                  *ctx.kind, 0, ptr(ws), ws.numel() * 4, stream_ptr()), bwd)
        return gtheta, gX, gY, None, None


def rbf_gram(theta, X, Y=None, y_shared=False):
    """theta (S,D+1); X (C,M,D); Y None | (C,N,D) | (N,D) with y_shared -> K (S,C,M,N)."""
    return _Gram.apply(theta, X, Y, y_shared, 0)


def matern_gram(theta, X, Y=None, y_shared=False, nu=2.5):
    """Matern kernel matrix, nu in {0.5, 1.5, 2.5}; arguments and result as rbf_gram."""
    if nu not in _MATERN_NU2:
        raise ValueError(f'matern_gram: nu must be 0.5, 1.5 or 2.5, got {nu!r}')
    return _Gram.apply(theta, X, Y, y_shared, _MATERN_NU2[nu])


# ------------------------------------------------------------------------------------------------
# Cholesky (+ jitter) with inverse factor
# ------------------------------------------------------------------------------------------------
def lazy_slot(n):
    """'lazy' mode: raise what earlier calls left behind, then hand out the next (pinned int32 host buffer, event) of the ring for n
    status words.  The caller gets the status words copied into the buffer and the event recorded behind them -- `_note_chol_errors`
    with a torch copy, the native programs by themselves (info_host / info_event: no torch launch at all) -- and appends the pair
    to `_pending`.  Buffers and events are recycled (allocating them per call cost ~40 us); every event has been recorded once,
    so that its native handle exists."""
    check_linalg_errors()
    ring = _lazy_rings.setdefault((torch.cuda.current_device(), n), [[], 0])       # (events belong to a device)
    if len(ring[0]) < 16:
        ev = torch.cuda.Event()
        ev.record()
        ring[0].append((torch.empty(n, dtype=torch.int32, pin_memory=True), ev))
    host, ev = ring[0][ring[1] % len(ring[0])]
    ring[1] += 1
    if any(h is host for h, _ in _pending):        # the ring has come round to a copy that has not been looked at: wait for it
        check_linalg_errors(wait=True)
    return host, ev


def raise_slot(n):
    """(pinned int32 host buffer of n status words, event) for the 'raise' mode, recycled per size.  The event has been recorded
    once, so that its native handle exists: the first-task program records it itself right behind its factorisation launch
    (include/vargp_hip.h: info_host / info_event) and the caller waits for THAT, not for the whole forward."""
    key = ('raise', torch.cuda.current_device(), n)                                 # (events belong to a device)
    slot = _lazy_rings.get(key)
    if slot is None:
        ev = torch.cuda.Event()
        ev.record()
        slot = _lazy_rings[key] = (torch.empty(n, dtype=torch.int32, pin_memory=True), ev)
    return slot


def _raise_if_bad(host):
    nz = host[host != 0]
    if nz.numel():
        raise torch.linalg.LinAlgError(
            f'vargp_chol_inv: {int(nz.numel())} of {host.numel()} matrices are not positive-definite '
            f'(first failing leading minor of order {int(nz[0])})')


def raise_wait(host, ev):
    ev.synchronize()
    _raise_if_bad(host)


def _note_chol_errors(info):
    if _chol_mode == 'lazy':
        host, ev = lazy_slot(info.numel())
        host.copy_(info.view(-1), non_blocking=True)
        ev.record()
        _pending.append((host, ev))
        return
    if _chol_mode == 'raise':
        # one copy into a (recycled) pinned buffer + an event wait: `(info != 0).sum().item()` was two reduction launches and a
        # synchronising read on every call
        if info.is_cuda:
            host, ev = raise_slot(info.numel())
            host.copy_(info.view(-1), non_blocking=True)
            ev.record()
            raise_wait(host, ev)
        else:
            _raise_if_bad(info.view(-1))
    else:
        _info_ring.append(info)
        del _info_ring[:-64]


class _CholInv(Function):
    @staticmethod
    def forward(ctx, A, eps, want_inv):
        require_device(A)
        ctx.set_materialize_grads(False)
        n = A.shape[-1]
        Ac = A.contiguous()
        nb = Ac.numel() // (n * n)
        L = torch.empty_like(Ac)
        need_T = want_inv or ctx.needs_input_grad[0]
        T = torch.empty_like(Ac) if need_T else None
        info = torch.empty(nb, dtype=torch.int32, device=A.device)
        ws = scratch(lib().vargp_chol_workspace_bytes(nb, n, 0), A.device)
        check(lib().vargp_chol_inv_fwd(ptr(Ac), float(eps), ptr(L), ptr(T), None, ptr(info), nb, n, ptr(ws),
                                       ws.numel() * 4, stream_ptr()), 'vargp_chol_inv_fwd')
        _note_chol_errors(info)
        ctx.save_for_backward(L, T)
        ctx.want_inv = want_inv
        if want_inv:
            return L, T
        dummy = L.new_empty(0)
        ctx.mark_non_differentiable(dummy)
        return L, dummy

    @staticmethod
    @once_differentiable
    def backward(ctx, gL, gT):
        L, T = ctx.saved_tensors
        if gL is None and (gT is None or not ctx.want_inv):
            return None, None, None
        n = L.shape[-1]
        nb = L.numel() // (n * n)
        gL = gL.contiguous() if gL is not None else None
        gT = gT.contiguous() if (ctx.want_inv and gT is not None) else None
        gA = torch.empty_like(L)
        ws = scratch(lib().vargp_chol_workspace_bytes(nb, n, 1), L.device)
        check(lib().vargp_chol_inv_bwd(ptr(L), ptr(T), ptr(gL), ptr(gT), ptr(gA), nb, n, ptr(ws), ws.numel() * 4,
                                       stream_ptr()), 'vargp_chol_inv_bwd')
        return gA, None, None


def chol_inv(A, eps=JITTER):
    """-> (L, T): L = chol(A + eps I) (lower), T = L^-1."""
    return _CholInv.apply(A, eps, True)


def chol(A, eps=JITTER):
    return _CholInv.apply(A, eps, False)[0]


# ------------------------------------------------------------------------------------------------
# packed triangle
# ------------------------------------------------------------------------------------------------
class _Vec2Tril(Function):
    @staticmethod
    def forward(ctx, vec, m):
        require_device(vec)
        vec = vec.contiguous()
        nb = vec.numel() // vec.shape[-1]
        out = torch.empty(*vec.shape[:-1], m, m, dtype=torch.float32, device=vec.device)
        check(lib().vargp_vec2tril_fwd(ptr(vec), ptr(out), nb, m, stream_ptr()), 'vargp_vec2tril_fwd')
        ctx.save_for_backward(vec)
        ctx.m = m
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        vec, = ctx.saved_tensors
        nb = vec.numel() // vec.shape[-1]
        gv = torch.empty_like(vec)
        check(lib().vargp_vec2tril_bwd(ptr(vec), ptr(g.contiguous()), ptr(gv), nb, ctx.m, stream_ptr()),
              'vargp_vec2tril_bwd')
        return gv, None


def vec2tril(vec, m):
    return _Vec2Tril.apply(vec, m)


def mat2trilvec(mat):
    require_device(mat)
    mat = mat.contiguous()
    m = mat.shape[-1]
    nb = mat.numel() // (m * m)
    out = torch.empty(*mat.shape[:-2], m * (m + 1) // 2, dtype=torch.float32, device=mat.device)
    check(lib().vargp_mat2trilvec(ptr(mat), ptr(out), nb, m, stream_ptr()), 'vargp_mat2trilvec')
    return out


# ------------------------------------------------------------------------------------------------
# predictive diag, MVN KL, log-det, likelihood
# ------------------------------------------------------------------------------------------------
class _PredictiveDiag(Function):
    @staticmethod
    def forward(ctx, P, W, a, kdiag):
        require_device(P, W, a, kdiag)
        P, W, a, kdiag = P.contiguous(), W.contiguous(), a.contiguous(), kdiag.contiguous()
        M, B = P.shape[-2:]
        nb = P.numel() // (M * B)
        mu = torch.empty(*P.shape[:-2], B, dtype=torch.float32, device=P.device)
        var = torch.empty_like(mu)
        check(lib().vargp_predictive_diag_fwd(ptr(P), ptr(W), ptr(a), 1, M, ptr(kdiag), ptr(mu), ptr(var), nb, M, B,
                                              stream_ptr()), 'vargp_predictive_diag_fwd')
        ctx.save_for_backward(P, W, a)
        return mu, var

    @staticmethod
    @once_differentiable
    def backward(ctx, gmu, gvar):
        P, W, a = ctx.saved_tensors
        M, B = P.shape[-2:]
        nb = P.numel() // (M * B)
        gP, gW, ga = torch.empty_like(P), torch.empty_like(W), torch.empty_like(a)
        gk = torch.empty(P.shape[:-2], dtype=torch.float32, device=P.device)
        check(lib().vargp_predictive_diag_bwd(ptr(P), ptr(W), ptr(a), 1, M, ptr(gmu.contiguous()), ptr(gvar.contiguous()),
                                              ptr(gP), ptr(gW), ptr(ga), ptr(gk), nb, M, B, stream_ptr()),
              'vargp_predictive_diag_bwd')
        return gP, gW, ga, gk


def predictive_diag(P, W, a, kdiag):
    """P, W (..., M, B); a (..., M); kdiag (...) -> mu, var (..., B)."""
    return _PredictiveDiag.apply(P, W, a, kdiag)


def predictive_cov(theta, X, P, W, nu2=0):
    """Full predictive covariance of one block of points (csrc/pred_cov.hip), no autograd:
    theta (S, D+1); X (B, D), shared by the classes; P, W (S, C, Mt, B) as for predictive_diag; nu2 0 (RBF) | 1 | 3 | 5
    (Matern, nu = nu2 / 2)  ->  Sigma (S, C, B, B) = K_theta(X, X) - P^T P + W^T W, bitwise symmetric, 4 S C B^2 bytes."""
    require_device(theta, X, P, W)
    theta, X, P, W = theta.detach().contiguous(), X.detach().contiguous(), P.detach().contiguous(), W.detach().contiguous()
    S, D = theta.shape[0], theta.shape[1] - 1
    B = X.shape[0]
    assert X.dim() == 2 and X.shape[1] == D, (X.shape, theta.shape)
    assert P.dim() == 4 and P.shape == W.shape and P.shape[0] == S and P.shape[-1] == B, (P.shape, W.shape, S, B)
    C, Mt = P.shape[1], P.shape[2]
    out = torch.empty(S, C, B, B, dtype=torch.float32, device=X.device)
    ws = scratch(lib().vargp_predictive_cov_workspace_bytes(S, B, D), X.device)
    check(lib().vargp_predictive_cov(ptr(theta), ptr(X), ptr(P), ptr(W), ptr(out), S, C, Mt, B, D, int(nu2), ptr(ws),
                                     ws.numel() * 4, stream_ptr()), 'vargp_predictive_cov')
    return out


def rff_paths(theta, X, omega, coef, x_shared):
    """Random-Fourier-feature paths (csrc/rff.hip), no autograd: theta (S, D+1); omega (R, D); coef (S, C, 2R, N);
    X (n, D) with x_shared (one point set for all outputs) or (C, n, D) without  ->  out (S, C, n, N) = Phi_s(X) coef[s, c] with
    Phi_s(X) = gamma_s / sqrt(R) [cos p | sin p], p = (X / lengthscale_s) omega^T.  The S n 2R features are never stored; two
    calls are bitwise equal."""
    require_device(theta, X, omega, coef)
    theta, X, omega, coef = (t.detach().contiguous() for t in (theta, X, omega, coef))
    assert all(t.dtype == torch.float32 for t in (theta, X, omega, coef)), (theta.dtype, X.dtype, omega.dtype, coef.dtype)
    S, D = theta.shape[0], theta.shape[1] - 1
    assert omega.dim() == 2 and omega.shape[1] == D, (omega.shape, theta.shape)
    R = omega.shape[0]
    assert coef.dim() == 4 and coef.shape[0] == S and coef.shape[2] == 2 * R, (coef.shape, S, R)
    C, N = coef.shape[1], coef.shape[3]
    if x_shared:
        assert X.dim() == 2 and X.shape[1] == D, (X.shape, theta.shape)
    else:
        assert X.dim() == 3 and X.shape[0] == C and X.shape[2] == D, (X.shape, C, D)
    n = X.shape[-2]
    out = torch.empty(S, C, n, N, dtype=torch.float32, device=X.device)
    ws = scratch(lib().vargp_rff_paths_workspace_bytes(S, D, R), X.device)
    check(lib().vargp_rff_paths(ptr(theta), ptr(X), ptr(omega), ptr(coef), ptr(out), S, C, n, D, R, N, int(bool(x_shared)),
                                ptr(ws), ws.numel() * 4, stream_ptr()), 'vargp_rff_paths')
    return out


class _RffPathsX(Function):
    @staticmethod
    def forward(ctx, theta, X, omega, coef, x_shared):
        out = rff_paths(theta, X, omega, coef, x_shared)
        ctx.save_for_backward(*(t.detach().contiguous() for t in (theta, X, omega, coef)))
        ctx.x_shared = bool(x_shared)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        theta, X, omega, coef = ctx.saved_tensors
        gout = gout.contiguous()
        S, D = theta.shape[0], theta.shape[1] - 1
        R, C, N, n = omega.shape[0], coef.shape[1], coef.shape[3], X.shape[-2]
        assert gout.dtype == torch.float32 and gout.shape == (S, C, n, N), (gout.dtype, gout.shape)
        gX = torch.empty_like(X)
        shared = int(ctx.x_shared)
        ws = scratch(lib().vargp_rff_paths_bwd_workspace_bytes(S, C, n, D, R, shared), X.device)
        check(lib().vargp_rff_paths_bwd(ptr(theta), ptr(X), ptr(omega), ptr(coef), ptr(gout), ptr(gX), S, C, n, D, R, N, shared,
                                        ptr(ws), ws.numel() * 4, stream_ptr()), 'vargp_rff_paths_bwd')
        return None, gX, None, None, None


def rff_paths_x(theta, X, omega, coef, x_shared):
    """rff_paths as an autograd node, differentiable in the points X only (theta, omega and coef get None): the forward is
    rff_paths itself, bit for bit; the backward is ONE fused kernel (csrc/rff.hip, vargp_rff_paths_bwd) that stores neither the
    phases, the features nor their gradient  ->  gX of X's shape.  Two backward calls are bitwise equal."""
    return _RffPathsX.apply(theta, X, omega, coef, x_shared)


# Lloyd's two steps for G sets of K centres over one data matrix (csrc/kmeans.hip -- not in the reference).  No autograd.

def _kmeans_args(X, Z):
    assert X.dim() == 2 and Z.dim() == 3 and Z.shape[-1] == X.shape[1], (X.shape, Z.shape)
    assert X.dtype == torch.float32 and Z.dtype == torch.float32, (X.dtype, Z.dtype)
    (N, D), (G, K) = X.shape, Z.shape[:2]
    return G, K, N, D, scratch(lib().vargp_kmeans_workspace_bytes(G, K, N, D), X.device)


def kmeans_assign(X, Z):
    """X (N, D), Z (G, K, D) -> label int32 (G, N): the nearest centre of set g in squared Euclidean distance (the smallest index
    on a tie), and dist2 (G, N): that distance, >= 0.  The N x K distances are never stored."""
    require_device(X, Z)
    X, Z = X.detach().contiguous(), Z.detach().contiguous()
    G, K, N, D, ws = _kmeans_args(X, Z)
    label = torch.empty(G, N, dtype=torch.int32, device=X.device)
    dist2 = torch.empty(G, N, dtype=torch.float32, device=X.device)
    check(lib().vargp_kmeans_assign(ptr(X), ptr(Z), ptr(label), ptr(dist2), G, K, N, D, ptr(ws), ws.numel() * 4, stream_ptr()),
          'vargp_kmeans_assign')
    return label, dist2


def kmeans_update(X, label, Z):
    """X (N, D), label int32 (G, N), Z (G, K, D) -> Z_new (G, K, D): the mean of the points of each label (a centre without points
    keeps its row of Z bit for bit), and count int32 (G, K).  Z itself is not modified.  Bitwise reproducible."""
    require_device(X, label, Z)
    X, label = X.detach().contiguous(), label.detach().contiguous()
    Z_new = Z.detach().clone(memory_format=torch.contiguous_format)
    G, K, N, D, ws = _kmeans_args(X, Z_new)
    assert label.dtype == torch.int32 and label.shape == (G, N), (label.dtype, label.shape, G, N)
    count = torch.empty(G, K, dtype=torch.int32, device=X.device)
    check(lib().vargp_kmeans_update(ptr(X), ptr(label), ptr(Z_new), ptr(count), G, K, N, D, ptr(ws), ws.numel() * 4, stream_ptr()),
          'vargp_kmeans_update')
    return Z_new, count


# Greedy conditional-variance selection: a pivoted Cholesky over G candidate sets (csrc/greedy.hip -- not in the reference).
# No autograd.

def greedy_select(theta, X, cand=None, LT0=None, d0=None, M=None, nu2=0, eps=JITTER, n_sets=None):
    """theta (D+1,): ONE hyper vector; X (N, D); cand int32 (G, Nc): row numbers into X, or None = rows 0..N-1 for each of
    n_sets sets (default 1, or LT0's).  LT0 (G, k0, Nc) with d0 (G, Nc): a factorisation already begun (both or neither).
    -> (pick int32 (G, M): POSITIONS in the candidate list, pivot (G, M): the residual variance at each pick before its
    downdate, LT (G, k0 + M, Nc): row k = the k-th Cholesky column over the candidates, d (G, Nc): the residual variances left).
    nu2: 0 = RBF, 1 | 3 | 5 = Matern.  eps: a candidate whose residual variance is not above it is never preferred and ends the
    selection when it is the best left (rows of zeros from there on); the default is the jitter chol_inv adds, below which a
    point adds nothing that factorisation can see.  M + 1 launches, no host synchronisation; bitwise reproducible."""
    require_device(theta, X, cand, LT0, d0)
    assert (LT0 is None) == (d0 is None), 'greedy_select: LT0 and d0 go together'
    assert M is not None, 'greedy_select: M'
    theta, X = theta.detach().contiguous().view(-1), X.detach().contiguous()
    assert X.dim() == 2 and theta.numel() == X.shape[1] + 1, (theta.shape, X.shape)
    assert X.dtype == torch.float32 and theta.dtype == torch.float32, (X.dtype, theta.dtype)
    N, D = X.shape
    if cand is not None:
        cand = cand.detach().contiguous()
        assert cand.dim() == 2 and cand.dtype == torch.int32, (cand.shape, cand.dtype)
        G, Nc = cand.shape
    else:
        G, Nc = int(n_sets if n_sets is not None else (LT0.shape[0] if LT0 is not None else 1)), N
    k0 = 0 if LT0 is None else LT0.shape[1]
    M = int(M)
    LT = torch.empty(G, k0 + M, Nc, dtype=torch.float32, device=X.device)
    d = torch.empty(G, Nc, dtype=torch.float32, device=X.device)
    if k0:
        assert tuple(LT0.shape) == (G, k0, Nc) and tuple(d0.shape) == (G, Nc), (LT0.shape, d0.shape, G, Nc)
        assert LT0.dtype == torch.float32 and d0.dtype == torch.float32, (LT0.dtype, d0.dtype)
        LT[:, :k0].copy_(LT0.detach())
        d.copy_(d0.detach())
    pick = torch.empty(G, M, dtype=torch.int32, device=X.device)
    pivot = torch.empty(G, M, dtype=torch.float32, device=X.device)
    ws = scratch(lib().vargp_greedy_workspace_bytes(G, Nc, D, k0 + M), X.device)
    check(lib().vargp_greedy_select(ptr(theta), ptr(X), ptr(cand), ptr(LT), ptr(d), ptr(pick), ptr(pivot), G, Nc, N, D, k0, M,
                                    int(nu2), float(eps), ptr(ws), ws.numel() * 4, stream_ptr()), 'vargp_greedy_select')
    return pick, pivot, LT, d


# Weighted moments of the cross-kernel over a data set (csrc/moments.hip -- not in the reference).  No autograd.

def _data_operands(theta, Z, X, alpha=None, Q=None):
    """The operands every data-set pass shares -- theta (D+1,), Z (G, Mt, D), X (N, D) and, for the site passes, alpha (G, Mt) and
    Q (G, Mt, Mt) -- detached, contiguous and checked -> (theta, Z, X, alpha, Q, (G, Mt, N, D))."""
    det = lambda t: None if t is None else t.detach().contiguous()
    theta, Z, X, alpha, Q = det(theta).view(-1), det(Z), det(X), det(alpha), det(Q)
    assert Z.dim() == 3 and X.dim() == 2 and Z.shape[-1] == X.shape[1] and theta.numel() == X.shape[1] + 1, (theta.shape, Z.shape, X.shape)
    (G, Mt, D), N = Z.shape, X.shape[0]
    if alpha is not None:
        assert tuple(alpha.shape) == (G, Mt) and tuple(Q.shape) == (G, Mt, Mt), (alpha.shape, Q.shape, G, Mt)
    assert all(t is None or t.dtype == torch.float32 for t in (theta, Z, X, alpha, Q)), [t.dtype for t in (theta, Z, X)]
    return theta, Z, X, alpha, Q, (G, Mt, N, D)


def _gram_moments(entry, theta, Z, X, w, y, nu2=0):
    """gram_moments (entry vargp_gram_moments) and gram_moments_v (vargp_gram_moments_v): y is the latter's v."""
    require_device(theta, Z, X, w, y)
    theta, Z, X, _, _, (G, Mt, N, D) = _data_operands(theta, Z, X)
    y = y.detach().contiguous()
    assert tuple(y.shape) == (G, N) and y.dtype == torch.float32, (y.shape, y.dtype, G, N)
    if w is not None:
        w = w.detach().contiguous()
        assert tuple(w.shape) == (G, N) and w.dtype == torch.float32, (w.shape, w.dtype)
    Phi = torch.empty(G, Mt, Mt, dtype=torch.float32, device=X.device)
    c = torch.empty(G, Mt, dtype=torch.float32, device=X.device)
    sums = torch.empty(G, 2, dtype=torch.float32, device=X.device)
    ws = scratch(lib().vargp_gram_moments_workspace_bytes(G, Mt, N, D), X.device)
    check(getattr(lib(), entry)(ptr(theta), ptr(Z), ptr(X), ptr(w), ptr(y), ptr(Phi), ptr(c), ptr(sums), G, Mt, N, D, int(nu2),
                                ptr(ws), ws.numel() * 4, stream_ptr()), entry)
    return Phi, c, sums


def gram_moments_chunks(G, Mt, N, D):
    """The number of chunks ops.gram_moments cuts N points into for this shape (= partials per output tile); the shapes alone
    decide it."""
    return int(lib().vargp_gram_moments_chunks(int(G), int(Mt), int(N), int(D)))


def gram_moments(theta, Z, X, w, y, nu2=0):
    """theta (D+1,): ONE hyper vector; Z (G, Mt, D); X (N, D) shared by the G outputs; w (G, N) or None = 1; y (G, N).  With
    k_n = k(Z_g, x_n): -> (Phi (G, Mt, Mt) = sum_n w_n k_n k_n^T, exactly symmetric; c (G, Mt) = sum_n w_n y_n k_n; sums (G, 2) =
    (sum_n w_n, sum_n w_n y_n^2)).  nu2: 0 = RBF, 1 | 3 | 5 = Matern.  K(Z, X) is never stored and the scratch does not grow with
    N; fp32 within a chunk of points, fp64 across chunks; bitwise reproducible."""
    return _gram_moments('vargp_gram_moments', theta, Z, X, w, y, nu2)


def gram_moments_bwd_chunks(G, Mt, N, D):
    """The number of chunks the backward of ops.gram_moments_diff cuts N points into; the shapes alone decide it."""
    return int(lib().vargp_gram_moments_bwd_chunks(int(G), int(Mt), int(N), int(D)))


def gram_moments_bwd(theta, Z, X, w, y, gPhi, gc, nu2=0):
    """The fused backward of gram_moments (csrc/moments.hip, vargp_gram_moments_bwd) for contiguous fp32 operands: gPhi (G, Mt,
    Mt), any matrix, and gc (G, Mt) -> (gZ (G, Mt, D), gtheta (D + 1,)) with gtheta[D] NOT written (it needs the forward's outputs:
    _GramMoments.backward).  K(Z, X) and its gradient are never stored; bitwise reproducible."""
    (G, Mt, D), N = Z.shape, X.shape[0]
    gZ = torch.empty_like(Z)
    gtheta = torch.empty(D + 1, dtype=torch.float32, device=Z.device)
    ws = scratch(lib().vargp_gram_moments_bwd_workspace_bytes(G, Mt, N, D), Z.device)
    check(lib().vargp_gram_moments_bwd(ptr(theta), ptr(Z), ptr(X), ptr(w), ptr(y), ptr(gPhi), ptr(gc), ptr(gZ), ptr(gtheta),
                                       G, Mt, N, D, int(nu2), ptr(ws), ws.numel() * 4, stream_ptr()), 'vargp_gram_moments_bwd')
    return gZ, gtheta


class _GramMoments(Function):
    @staticmethod
    def forward(ctx, theta, Z, X, w, y, nu2):
        Phi, c, sums = gram_moments(theta, Z, X, w, y, nu2)
        det = lambda t: None if t is None else t.detach().contiguous()
        ctx.save_for_backward(det(theta).view(-1), det(Z), det(X), det(w), det(y), Phi, c)
        ctx.nu2, ctx.theta_shape = int(nu2), theta.shape
        ctx.mark_non_differentiable(sums)
        return Phi, c, sums

    @staticmethod
    @once_differentiable
    def backward(ctx, gPhi, gc, _gsums):
        theta, Z, X, w, y, Phi, c = ctx.saved_tensors
        gPhi = torch.zeros_like(Phi) if gPhi is None else gPhi.to(torch.float32).contiguous()
        gc = torch.zeros_like(c) if gc is None else gc.to(torch.float32).contiguous()
        gZ, gtheta = gram_moments_bwd(theta, Z, X, w, y, gPhi, gc, ctx.nu2)
        # the log-gamma entry needs no pass over the data: K is gamma^2 times a function of the distances, so
        # gtheta_D = 2 sum gK o K = 4 <gPhi, Phi> + 2 <gc, c>
        gtheta[-1] = (4.0 * (gPhi.double() * Phi.double()).sum() + 2.0 * (gc.double() * c.double()).sum()).float()
        return gtheta.view(ctx.theta_shape), gZ, None, None, None, None


def refuse_grad(who, produced, **data):
    """ValueError if one of the named data tensors requires grad: `who` produces gradients for `produced` only."""
    for name, t in data.items():
        if t is not None and t.requires_grad:
            raise ValueError(f'{who}: {name} requires grad, but gradients are produced for {produced} only')


def gram_moments_diff(theta, Z, X, w, y, nu2=0):
    """ops.gram_moments on the autograd graph of theta (D+1,) and Z (G, Mt, D): the same forward call and outputs (Phi, c, sums),
    with a fused backward that never stores K(Z, X) either (gram_moments_bwd).  gPhi may be any matrix (it is not assumed
    symmetric).  No gradients are produced for X, w and y: a ValueError if one of them requires grad.  sums depends on w and y
    alone and is not differentiable."""
    refuse_grad('gram_moments_diff', 'theta and Z', X=X, w=w, y=y)
    return _GramMoments.apply(theta, Z, X, w, y, nu2)


# Gaussian sites of a non-Gaussian likelihood over a data set (csrc/sites.hip -- not in the reference).  No autograd.
SITE_MAX_MT = 256                # kSiMaxMt (csrc/dataset_pass.h): the fused pass holds all Mt rows of a K block in LDS
SITE_BOUND_GRADS = 'theta, Z, alpha, Q and the Student-t log_scale'      # what the site bound's two routes differentiate
_SITE_KINDS = {('bernoulli', 0): 0, ('bernoulli', 1): 1, ('poisson', None): 2, ('studentt', None): 3}


def site_kind(kind, extra):
    """The VARGP_SITE_* code of a likelihood kind with its `extra` (as ops.lik_nll_fwd takes it) -> (code, log_scale, df,
    lognorm); ValueError for a kind without independent non-Gaussian sites."""
    if kind == 'bernoulli':
        return _SITE_KINDS[(kind, int(extra[0]))], None, 0.0, 0.0
    if kind == 'poisson':
        return _SITE_KINDS[(kind, None)], None, 0.0, 0.0
    if kind == 'studentt':
        return _SITE_KINDS[(kind, None)], extra[0], float(extra[1]), float(extra[2])
    raise ValueError(f"site_moments: kind must be 'bernoulli', 'poisson' or 'studentt', got {kind!r}")


def _site_operands(theta, Z, X, alpha, Q, y, w, kind, extra):
    """The operands of the two site entries, detached, contiguous and checked -> (theta, Z, X, alpha, Q, yt, ldy, w, code,
    log_scale, df, lognorm, (G, Mt, N, D))."""
    code, log_scale, df, lognorm = site_kind(kind, extra)
    theta, Z, X, alpha, Q, (G, Mt, N, D) = _data_operands(theta, Z, X, alpha, Q)
    yt, ldy = reg_target(y, G, N)
    if w is not None:
        w = w.detach().contiguous()
        assert tuple(w.shape) == (G, N) and w.dtype == torch.float32, (w.shape, w.dtype)
    if log_scale is not None:
        log_scale = log_scale.detach().contiguous()
        assert tuple(log_scale.shape) == (G,) and log_scale.dtype == torch.float32, (log_scale.shape, log_scale.dtype)
    return theta, Z, X, alpha, Q, yt, ldy, w, code, log_scale, df, lognorm, (G, Mt, N, D)


def site_moments_chunks(G, Mt, N, D):
    """The number of chunks ops.site_moments cuts N points into for this shape; the shapes alone decide it."""
    return int(lib().vargp_site_moments_chunks(int(G), int(Mt), int(N), int(D)))


def site_moments(theta, Z, X, alpha, Q, y, w, kind, extra=(), nu2=0):
    """theta (D+1,): ONE hyper vector; Z (G, Mt, D), Mt <= SITE_MAX_MT; X (N, D) shared by the G outputs; alpha (G, Mt) and a
    symmetric Q (G, Mt, Mt): q(f_n) = N(alpha . k_n, max(gamma^2 - k_n^T Q k_n, 0)), k_n = k(Z_g, x_n); y (G, N) or (N,) (one row
    for every output), targets as the kind's nll reads float targets; w (G, N) or None = 1; kind / extra: as ops.lik_nll_fwd
    names the likelihood ('bernoulli' (link code,), 'poisson' (), 'studentt' (log_scale (G,), df, lognorm)).
    -> (lam2 (G, N) = w max(-2 d ell / d var, 0); c (G, Mt) = sum_n (w d ell / d mu + lam2 mu_n) k_n; sums (G, 4) = (sum w ell,
    sum lam2, clamped points, sum w)).  K(Z, X) is never stored and the scratch does not grow with N beyond the chunk count;
    bitwise reproducible; a point of weight 0 adds exactly nothing."""
    require_device(theta, Z, X, alpha, Q, y, w)
    theta, Z, X, alpha, Q, yt, ldy, w, code, log_scale, df, lognorm, (G, Mt, N, D) = _site_operands(theta, Z, X, alpha, Q, y, w, kind, extra)
    lam2 = torch.empty(G, N, dtype=torch.float32, device=X.device)
    c = torch.empty(G, Mt, dtype=torch.float32, device=X.device)
    sums = torch.empty(G, 4, dtype=torch.float32, device=X.device)
    ws = scratch(lib().vargp_site_moments_workspace_bytes(G, Mt, N, D), X.device)
    check(lib().vargp_site_moments(ptr(theta), ptr(Z), ptr(X), ptr(alpha), ptr(Q), ptr(yt), ldy, ptr(w), code, ptr(log_scale), df,
                                   lognorm, ptr(lam2), ptr(c), ptr(sums), G, Mt, N, D, int(nu2), ptr(ws), ws.numel() * 4,
                                   stream_ptr()), 'vargp_site_moments')
    return lam2, c, sums


# The data passes of the softmax site iteration (csrc/sites.hip, csrc/softmax_sites.hip, csrc/moments.hip -- not in the
# reference).  No autograd.
SOFTMAX_SITE_MAX_C = 128         # kSmMaxC (csrc/softmax_sites.hip)


def site_marginals(theta, Z, X, alpha, Q, nu2=0):
    """The marginals of q(f) at every point: theta, Z (G, Mt, D), Mt <= SITE_MAX_MT, X (N, D), alpha (G, Mt) and a symmetric Q (G,
    Mt, Mt) as site_moments takes them -> (mu (G, N) = alpha . k_n, var (G, N) = max(gamma^2 - k_n^T Q k_n, 0)).  site_moments'
    kernel stopped after the marginals (vargp_site_marginals): K(Z, X) is never stored, no workspace, bitwise reproducible."""
    require_device(theta, Z, X, alpha, Q)
    theta, Z, X, alpha, Q, (G, Mt, N, D) = _data_operands(theta, Z, X, alpha, Q)
    mu = torch.empty(G, N, dtype=torch.float32, device=X.device)
    var = torch.empty(G, N, dtype=torch.float32, device=X.device)
    check(lib().vargp_site_marginals(ptr(theta), ptr(Z), ptr(X), ptr(alpha), ptr(Q), ptr(mu), ptr(var), G, Mt, N, D, int(nu2),
                                     stream_ptr()), 'vargp_site_marginals')
    return mu, var


# The leave-one-out cavity of the Gaussian sites (csrc/sites.hip: vargp_site_cavity -- not in the reference).  No autograd.
SiteCavity = namedtuple('SiteCavity', 'mu_c var_c lam1 lam2 n_unstable mu var s')
SiteCavity.__doc__ = """mu_c, var_c (G, N): the cavity moments, NaN at an unstable point; lam1, lam2 (G, N): the sites; n_unstable
(G,) int64; mu, var, s (G, N): the marginals of q(f) and s_n = |V k_n|^2, as the same launch wrote them."""


def _cavity_V(V, G, Mt):
    V = V.detach().contiguous()
    assert V.dim() == 3 and V.shape[0] == G and V.shape[2] == Mt and 1 <= V.shape[1] <= Mt and V.dtype == torch.float32, \
        (V.shape, V.dtype, G, Mt)
    return V


def site_cavity_chunks(G, Mt, N, D):
    """The number of chunks ops.site_cavity cuts N points into for this shape: site_moments'."""
    return int(lib().vargp_site_cavity_chunks(int(G), int(Mt), int(N), int(D)))


def site_marginals_s(theta, Z, X, alpha, Q, V, nu2=0):
    """site_marginals, and the share of the variance that one block of q owns: V (G, Mv, Mt), Mv <= Mt -> (mu (G, N), var (G, N),
    s (G, N) = |V k_n|^2).  The marginals form of vargp_site_cavity: V K runs on the MFMA in the registers of Q K and only its
    column norms leave the kernel; no workspace, bitwise reproducible."""
    require_device(theta, Z, X, alpha, Q, V)
    theta, Z, X, alpha, Q, (G, Mt, N, D) = _data_operands(theta, Z, X, alpha, Q)
    V = _cavity_V(V, G, Mt)
    mu, var, s = (torch.empty(G, N, dtype=torch.float32, device=X.device) for _ in range(3))
    check(lib().vargp_site_cavity(ptr(theta), ptr(Z), ptr(X), ptr(alpha), ptr(Q), ptr(V), None, 0, None, -1, None, 0.0, 0.0,
                                  ptr(mu), ptr(var), ptr(s), None, None, None, None, None, G, Mt, V.shape[1], N, D, int(nu2),
                                  None, 0, stream_ptr()), 'vargp_site_cavity')
    return mu, var, s


def site_cavity(theta, Z, X, alpha, Q, V, y, w, kind, extra=(), nu2=0):
    """The Gaussian sites of site_moments at q(f_n) = N(alpha . k_n, max(gamma^2 - k_n^T Q k_n, 0)) and the cavity each leaves when it
    is divided out of the block of q that V (G, Mv, Mt) describes; the other operands as site_moments takes them.  With s_n =
    |V k_n|^2 and r_n = 1 - lam2_n s_n: mu_c = (mu - s lam1) / r, var_c = var + lam2 s^2 / r, in fp64 from the fp32 moments.  A
    point with r <= 0 or a non-finite result is unstable: NaN, and counted; a point of weight 0 has lam = 0 and the cavity
    (mu, var) exactly.  -> SiteCavity(mu_c, var_c, lam1, lam2, n_unstable (G,) int64, mu, var, s).  One fused launch plus the
    reduce of the counts; K(Z, X) and V K are never stored; bitwise reproducible."""
    require_device(theta, Z, X, alpha, Q, V, y, w)
    theta, Z, X, alpha, Q, yt, ldy, w, code, log_scale, df, lognorm, (G, Mt, N, D) = _site_operands(theta, Z, X, alpha, Q, y, w, kind, extra)
    V = _cavity_V(V, G, Mt)
    mu, var, s, mu_c, var_c, lam1, lam2 = (torch.empty(G, N, dtype=torch.float32, device=X.device) for _ in range(7))
    n_unstable = torch.empty(G, dtype=torch.int64, device=X.device)
    ws = scratch(lib().vargp_site_cavity_workspace_bytes(G, Mt, N, D), X.device)
    check(lib().vargp_site_cavity(ptr(theta), ptr(Z), ptr(X), ptr(alpha), ptr(Q), ptr(V), ptr(yt), ldy, ptr(w), code, ptr(log_scale),
                                  df, lognorm, ptr(mu), ptr(var), ptr(s), ptr(mu_c), ptr(var_c), ptr(lam1), ptr(lam2), ptr(n_unstable),
                                  G, Mt, V.shape[1], N, D, int(nu2), ptr(ws), ws.numel() * 4, stream_ptr()), 'vargp_site_cavity')
    return SiteCavity(mu_c, var_c, lam1, lam2, n_unstable, mu, var, s)


def _seed64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def softmax_site_noise(seed, n_f, C, N, device=None):
    """The standard-normal draws (n_f, C, N) that softmax_sites(eps=None, seed=seed) generates inside its kernel
    (vargp_softmax_site_noise): Philox group (n n_f + f) ceil(C / 4) + j of noise stream 2, element l of group j for class 4 j + l."""
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != 'cuda':
        raise _lib.VargpHipError('vargp_amd ops need a ROCm device (cuda:N); there is no CPU path in the product')
    eps = torch.empty(int(n_f), int(C), int(N), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        check(lib().vargp_softmax_site_noise(_seed64(seed), ptr(eps), int(n_f), int(C), int(N), stream_ptr()),
              'vargp_softmax_site_noise')
    return eps


def _softmax_operands(mu, var, y, w, eps, n_f):
    """The operands of the two softmax site entries, detached, contiguous and checked -> (mu, var, y, w, eps, C, N, F)."""
    det = lambda t: t.detach().contiguous()
    mu, var, y = det(mu), det(var), det(y)
    assert mu.dim() == 2 and mu.shape == var.shape and mu.dtype == var.dtype == torch.float32, (mu.shape, var.shape, mu.dtype, var.dtype)
    C, N = mu.shape
    F = int(n_f)
    assert tuple(y.shape) == (N,) and y.dtype == torch.int64, (y.shape, y.dtype)
    if w is not None:
        w = det(w)
        assert tuple(w.shape) == (N,) and w.dtype == torch.float32, (w.shape, w.dtype)
    if eps is not None:
        eps = det(eps)
        assert tuple(eps.shape) == (F, C, N) and eps.dtype == torch.float32, (eps.shape, eps.dtype, (F, C, N))
    return mu, var, y, w, eps, C, N, F


def softmax_sites(mu, var, y, w, n_f, seed=0, eps=None):
    """The Gaussian sites of the softmax likelihood at the marginals mu, var (C, N) fp32 of q(f): y (N,) int64 class indices, w
    (N,) or None = 1, n_f Monte-Carlo draws per point -- eps (n_f, C, N) if given, else generated in the kernel from `seed` (the
    draws softmax_site_noise(seed, n_f, C, N) returns; bitwise the same result).  With p = softmax(mu + sqrt(var) eps):
    -> (lam1 (C, N) = w ([y = c] - E p_c) + lam2 mu, lam2 (C, N) = w E p_c (1 - p_c) >= 0, sums (4,) = (sum_n w ell, sum lam2,
    #{w != 0}, sum w)), ell_n = mu[y_n, n] - E logsumexp(f).  2 <= C <= SOFTMAX_SITE_MAX_C; a point of weight 0 is not evaluated
    and adds exactly nothing; bitwise reproducible."""
    require_device(mu, var, y, w, eps)
    mu, var, y, w, eps, C, N, F = _softmax_operands(mu, var, y, w, eps, n_f)
    lam1, lam2 = torch.empty_like(mu), torch.empty_like(mu)
    sums = torch.empty(4, dtype=torch.float32, device=mu.device)
    ws = scratch(lib().vargp_softmax_sites_workspace_bytes(C, N), mu.device)
    check(lib().vargp_softmax_sites(ptr(mu), ptr(var), ptr(y), ptr(w), ptr(eps), _seed64(seed), ptr(lam1), ptr(lam2), ptr(sums),
                                    C, N, F, ptr(ws), ws.numel() * 4, stream_ptr()), 'vargp_softmax_sites')
    return lam1, lam2, sums


def gram_moments_v(theta, Z, X, w, v, nu2=0):
    """gram_moments with a weight vector of its own for c: w (G, N) or None = 1 and v (G, N) -> (Phi (G, Mt, Mt) = sum_n w_n k_n
    k_n^T, c (G, Mt) = sum_n v_n k_n, sums (G, 2) = (sum w, sum v)).  The same kernel, chunking and scratch; with v = w * y, Phi
    and c are bitwise gram_moments'."""
    return _gram_moments('vargp_gram_moments_v', theta, Z, X, w, v, nu2)


def site_bound_bwd_chunks(G, Mt, N, D):
    """The number of chunks ops.site_bound_bwd cuts N points into for this shape; the shapes alone decide it."""
    return int(lib().vargp_site_bound_bwd_chunks(int(G), int(Mt), int(N), int(D)))


def _site_bwd_outputs(workspace_bytes, Z, N):
    """What the two fused backward entries of the site passes write: -> (gZ (G, Mt, D), gtheta (D + 1,), galpha (G, Mt), gv (G, N),
    the entry's workspace)."""
    G, Mt, D = Z.shape
    gtheta = torch.empty(D + 1, dtype=torch.float32, device=Z.device)
    galpha = torch.empty(G, Mt, dtype=torch.float32, device=Z.device)
    gv = torch.empty(G, N, dtype=torch.float32, device=Z.device)
    return torch.empty_like(Z), gtheta, galpha, gv, scratch(workspace_bytes(G, Mt, N, D), Z.device)


def site_bound_bwd(theta, Z, X, alpha, Q, y, w, kind, extra, gout, nu2=0):
    """The fused backward of site_moments' sums[:, 0] (csrc/sites.hip, vargp_site_bound_bwd); operands as site_moments takes them
    and gout (G,), the seed of every output.  -> (gZ (G, Mt, D), gtheta (D + 1,), complete; galpha (G, Mt); gv (G, N) = seed x w x
    the TRUE d ell / d var, 0 where the variance is clamped: gQ = -gram_moments(w=gv).Phi; gls (G,) for Student-t, else None).
    K(Z, X) and its gradient are never stored; bitwise reproducible; a point of weight 0 adds exactly nothing."""
    require_device(theta, Z, X, alpha, Q, y, w, gout)
    theta, Z, X, alpha, Q, yt, ldy, w, code, log_scale, df, lognorm, (G, Mt, N, D) = _site_operands(theta, Z, X, alpha, Q, y, w, kind, extra)
    gout = gout.detach().contiguous()
    assert tuple(gout.shape) == (G,) and gout.dtype == torch.float32, (gout.shape, gout.dtype)
    gls = None if log_scale is None else torch.empty(G, dtype=torch.float32, device=X.device)
    gZ, gtheta, galpha, gv, ws = _site_bwd_outputs(lib().vargp_site_bound_bwd_workspace_bytes, Z, N)
    check(lib().vargp_site_bound_bwd(ptr(theta), ptr(Z), ptr(X), ptr(alpha), ptr(Q), ptr(yt), ldy, ptr(w), code, ptr(log_scale), df,
                                     lognorm, ptr(gout), ptr(gZ), ptr(gtheta), ptr(galpha), ptr(gv), ptr(gls), G, Mt, N, D,
                                     int(nu2), ptr(ws), ws.numel() * 4, stream_ptr()), 'vargp_site_bound_bwd')
    return gZ, gtheta, galpha, gv, gls


def _bound_grads(ctx, theta, Z, X, gZ, gtheta, galpha, gv, gown=None):
    """The tail of both bound nodes' backward: gQ = -gram_moments(w = gv).Phi, and the gradients of the eleven forward arguments
    (theta, Z, X, alpha, Q, y, w, the eighth -- log_scale, with gradient gown, or eps --, three constants)."""
    gQ = -gram_moments(theta, Z, X, gv, gv, ctx.nu2)[0]
    return gtheta.view(ctx.theta_shape), gZ, None, galpha, gQ, None, None, gown, None, None, None


class _SiteBound(Function):
    @staticmethod
    def forward(ctx, theta, Z, X, alpha, Q, y, w, log_scale, kind, extra, nu2):
        det = lambda t: None if t is None else t.detach().contiguous()
        extra = tuple(extra) if log_scale is None else (det(log_scale),) + tuple(extra[1:])
        value = site_moments(theta, Z, X, alpha, Q, y, w, kind, extra, nu2)[2][:, 0].contiguous()
        ctx.save_for_backward(det(theta).view(-1), det(Z), det(X), det(alpha), det(Q), det(y), det(w), det(log_scale))
        ctx.kind, ctx.extra, ctx.nu2, ctx.theta_shape = kind, extra, int(nu2), theta.shape
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        theta, Z, X, alpha, Q, y, w, log_scale = ctx.saved_tensors
        gout = gout.to(torch.float32).contiguous()
        return _bound_grads(ctx, theta, Z, X, *site_bound_bwd(theta, Z, X, alpha, Q, y, w, ctx.kind, ctx.extra, gout, ctx.nu2))


def site_bound_diff(theta, Z, X, alpha, Q, y, w, kind, extra=(), nu2=0):
    """value (G,) = sum_n w_n E_{q(f_n)} log p(y_n | f_n) = site_moments(...)[2][:, 0] (the same forward call, bitwise) on the
    autograd graph of theta (D+1,), Z (G, Mt, D), alpha (G, Mt), Q (G, Mt, Mt) (through its symmetric part; the variance clamp
    passes no gradient) and, for Student-t, extra[0] = log_scale (G,).  The backward is one fused pass (site_bound_bwd) and one
    gram_moments call for gQ; K(Z, X) is never stored in either.  No gradients are produced for X, y and w: a ValueError if one
    of them requires grad."""
    refuse_grad('site_bound_diff', SITE_BOUND_GRADS, X=X, y=y, w=w)
    log_scale = extra[0] if kind == 'studentt' else None
    return _SiteBound.apply(theta, Z, X, alpha, Q, y, w, log_scale, kind, tuple(extra), nu2)


# The softmax site bound on the autograd graph (csrc/softmax_sites.hip: vargp_softmax_site_grads; csrc/sites.hip:
# vargp_site_transport_bwd -- not in the reference).
SOFTMAX_BOUND_GRADS = 'theta, Z, alpha and Q'


def softmax_site_grads(mu, var, y, w, n_f, gout, seed=0, eps=None):
    """The exact derivatives of softmax_sites(...)[2][0] -- the n_f-sample estimate sum_n w_n (mu[y_n, n] - mean_f logsumexp(f)) --
    for the marginals, operands as softmax_sites takes them and gout (1,) fp32 on the device, the upstream seed:
    -> (gmu (C, N) = gout w ([y = c] - mean_f p_c), gvar (C, N) = -gout w mean_f (p_c eps_c) / (2 sqrt(var)), exactly 0 where var
    == 0).  The pathwise derivative for var, not the Price estimate behind lam2.  The same draws as softmax_sites (eps or seed,
    bitwise alike); a point of weight 0 is not evaluated and gets exact zeros; no workspace; bitwise reproducible."""
    require_device(mu, var, y, w, eps, gout)
    mu, var, y, w, eps, C, N, F = _softmax_operands(mu, var, y, w, eps, n_f)
    gout = gout.detach().contiguous().view(-1)
    assert gout.numel() == 1 and gout.dtype == torch.float32, (gout.shape, gout.dtype)
    gmu, gvar = torch.empty_like(mu), torch.empty_like(mu)
    check(lib().vargp_softmax_site_grads(ptr(mu), ptr(var), ptr(y), ptr(w), ptr(eps), _seed64(seed), ptr(gout), ptr(gmu), ptr(gvar),
                                         C, N, F, stream_ptr()), 'vargp_softmax_site_grads')
    return gmu, gvar


def site_transport_bwd_chunks(G, Mt, N, D):
    """The number of chunks ops.site_transport_bwd cuts N points into for this shape (site_bound_bwd's rule)."""
    return int(lib().vargp_site_transport_bwd_chunks(int(G), int(Mt), int(N), int(D)))


def site_transport_bwd(theta, Z, X, alpha, Q, gm, gv, nu2=0):
    """site_bound_bwd with GIVEN per-point seeds in place of a likelihood (csrc/sites.hip, vargp_site_transport_bwd): theta, Z, X,
    alpha, Q as site_marginals takes them; gm, gv (G, N) = d value / d mu, d value / d var of every point (weights and upstream
    seed included).  -> (gZ (G, Mt, D); gtheta (D + 1,), complete; galpha (G, Mt); gv_out (G, N) = gv where gamma^2 - k^T Q k > 0,
    else 0: gQ = -gram_moments(w=gv_out).Phi).  K(Z, X) and its gradient are never stored; bitwise reproducible; a point whose gm
    and gv are both 0 adds exactly nothing whatever its row of X holds."""
    require_device(theta, Z, X, alpha, Q, gm, gv)
    theta, Z, X, alpha, Q, (G, Mt, N, D) = _data_operands(theta, Z, X, alpha, Q)
    gm, gv = gm.detach().contiguous(), gv.detach().contiguous()
    assert tuple(gm.shape) == tuple(gv.shape) == (G, N) and gm.dtype == gv.dtype == torch.float32, (gm.shape, gv.shape, gm.dtype)
    gZ, gtheta, galpha, gv_out, ws = _site_bwd_outputs(lib().vargp_site_transport_bwd_workspace_bytes, Z, N)
    check(lib().vargp_site_transport_bwd(ptr(theta), ptr(Z), ptr(X), ptr(alpha), ptr(Q), ptr(gm), ptr(gv), ptr(gZ), ptr(gtheta),
                                         ptr(galpha), ptr(gv_out), G, Mt, N, D, int(nu2), ptr(ws), ws.numel() * 4, stream_ptr()),
          'vargp_site_transport_bwd')
    return gZ, gtheta, galpha, gv_out


class _SoftmaxSiteBound(Function):
    @staticmethod
    def forward(ctx, theta, Z, X, alpha, Q, y, w, eps, n_f, seed, nu2):
        det = lambda t: None if t is None else t.detach().contiguous()
        mu, var = site_marginals(theta, Z, X, alpha, Q, nu2)
        value = softmax_sites(mu, var, y, w, n_f, seed, eps)[2][:1].contiguous()
        ctx.save_for_backward(det(theta).view(-1), det(Z), det(X), det(alpha), det(Q), det(y), det(w), det(eps), mu, var)
        ctx.n_f, ctx.seed, ctx.nu2, ctx.theta_shape = int(n_f), seed, int(nu2), theta.shape
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        theta, Z, X, alpha, Q, y, w, eps, mu, var = ctx.saved_tensors
        gmu, gvar = softmax_site_grads(mu, var, y, w, ctx.n_f, gout.to(torch.float32).contiguous(), ctx.seed, eps)
        return _bound_grads(ctx, theta, Z, X, *site_transport_bwd(theta, Z, X, alpha, Q, gmu, gvar, ctx.nu2))


def softmax_site_bound_diff(theta, Z, X, alpha, Q, y, w, n_f, seed=0, eps=None, nu2=0):
    """value (1,) = sum_n w_n (mu[y_n, n] - mean_f logsumexp(mu_n + sqrt(var_n) eps_nf)) at the marginals of q(f) -- site_marginals
    followed by softmax_sites, its sums[0] bitwise -- on the autograd graph of theta (D+1,), Z (C, Mt, D), alpha (C, Mt) and Q (C,
    Mt, Mt) (through its symmetric part; the variance clamp passes no gradient).  y (N,) int64, w (N,) or None, n_f draws per point
    fixed by `seed` (or eps (n_f, C, N)).  mu and var (2 C N floats) are kept for the backward: softmax_site_grads (the exact
    derivative of the sampled value), site_transport_bwd and one gram_moments call for gQ; K(Z, X) is never stored.  No
    gradients are produced for X, y and w: a ValueError if one of them requires grad."""
    refuse_grad('softmax_site_bound_diff', SOFTMAX_BOUND_GRADS, X=X, y=y, w=w)
    return _SoftmaxSiteBound.apply(theta, Z, X, alpha, Q, y, w, eps, n_f, seed, nu2)


class _LogdetTril(Function):
    @staticmethod
    def forward(ctx, L):
        require_device(L)
        L = L.contiguous()
        n = L.shape[-1]
        nb = L.numel() // (n * n)
        out = torch.empty(L.shape[:-2], dtype=torch.float32, device=L.device)
        check(lib().vargp_logdet_tril_fwd(ptr(L), ptr(out), nb, n, stream_ptr()), 'vargp_logdet_tril_fwd')
        ctx.save_for_backward(L)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        L, = ctx.saved_tensors
        n = L.shape[-1]
        nb = L.numel() // (n * n)
        gL = torch.empty_like(L)
        check(lib().vargp_logdet_tril_bwd(ptr(L), ptr(g.contiguous()), ptr(gL), nb, n, stream_ptr()),
              'vargp_logdet_tril_bwd')
        return gL


def logdet_tril(L):
    return _LogdetTril.apply(L)


class _MvnKl(Function):
    @staticmethod
    def forward(ctx, G, d, ldp, ldq):
        require_device(G, d, ldp, ldq)
        G, d, ldp, ldq = G.contiguous(), d.contiguous(), ldp.contiguous(), ldq.contiguous()
        M = G.shape[-1]
        nb = G.numel() // (M * M)
        kl = torch.empty(G.shape[:-2], dtype=torch.float32, device=G.device)
        check(lib().vargp_mvn_kl_fwd(ptr(G), ptr(d), ptr(ldp), ptr(ldq), ptr(kl), nb, M, stream_ptr()),
              'vargp_mvn_kl_fwd')
        ctx.save_for_backward(G, d)
        return kl

    @staticmethod
    @once_differentiable
    def backward(ctx, gkl):
        G, d = ctx.saved_tensors
        M = G.shape[-1]
        nb = G.numel() // (M * M)
        gkl = gkl.contiguous()
        gG, gd = torch.empty_like(G), torch.empty_like(d)
        check(lib().vargp_mvn_kl_bwd(ptr(G), ptr(d), ptr(gkl), ptr(gG), ptr(gd), nb, M, stream_ptr()),
              'vargp_mvn_kl_bwd')
        return gG, gd, gkl, -gkl


def mvn_kl_from_factors(G, d, logdet_p, logdet_q):
    """KL per batch element from G = Lp^-1 Lq (..., M, M), d = Lp^-1 (mu_q - mu_p) (..., M) and the two
    log-dets (...)."""
    return _MvnKl.apply(G, d, logdet_p, logdet_q)


class _SoftmaxNll(Function):
    @staticmethod
    def forward(ctx, mu, var, eps, y):
        require_device(mu, var, eps, y)
        mu, var, eps, y = mu.contiguous(), var.contiguous(), eps.contiguous(), y.contiguous()
        assert y.dtype == torch.int64
        S, F, C, B = eps.shape
        assert mu.shape == (S, C, B) and var.shape == (S, C, B), (mu.shape, eps.shape)
        nll = torch.empty((), dtype=torch.float32, device=mu.device)
        check(lib().vargp_softmax_nll_fwd(ptr(mu), ptr(var), ptr(eps), ptr(y), ptr(nll), S, F, C, B, stream_ptr()),
              'vargp_softmax_nll_fwd')
        ctx.save_for_backward(mu, var, eps, y)
        return nll

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        mu, var, eps, y = ctx.saved_tensors
        S, F, C, B = eps.shape
        gmu, gvar = torch.empty_like(mu), torch.empty_like(var)
        check(lib().vargp_softmax_nll_bwd(ptr(mu), ptr(var), ptr(eps), ptr(y), ptr(g.contiguous()), ptr(gmu),
                                          ptr(gvar), S, F, C, B, stream_ptr()), 'vargp_softmax_nll_bwd')
        return gmu, gvar, None, None


def softmax_nll(mu, var, eps, y):
    return _SoftmaxNll.apply(mu, var, eps, y)


def softmax_predict(mu, var, eps):
    require_device(mu, var, eps)
    mu, var, eps = mu.contiguous(), var.contiguous(), eps.contiguous()
    S, F, C, B = eps.shape
    probs = torch.empty(B, C, dtype=torch.float32, device=mu.device)
    check(lib().vargp_softmax_predict(ptr(mu), ptr(var), ptr(eps), ptr(probs), S, F, C, B, stream_ptr()),
          'vargp_softmax_predict')
    return probs



# ------------------------------------------------------------------------------------------------
# Likelihoods with independent outputs -- Gaussian (csrc/gauss_lik.hip), Bernoulli / Poisson / Student-t (csrc/indep_lik.hip;
# not in the reference) -- and every likelihood's held-out log predictive density (csrc/lpd.hip; not in the reference, no
# autograd).  Their C ABI is uniform, so ONE table-driven call serves them all:
#   vargp_<kind>_nll_fwd(mu, var, <target...>, <extra...>, nll, S, C, B, [ws, ws_bytes], stream)
#   vargp_<kind>_nll_bwd(mu, var, <target...>, <extra...>, seed, gmu, gvar, [g_param], nll, S, C, B, [ws, ws_bytes], stream)
#   vargp_<kind>_lpd    (mu, var, <target...>, <extra...>, lpd, lpd_out, S, C, B, stream)
# target: the tuple from the kind's *_target;  extra: the output's own parameter (C,) and / or host constants --
#   gauss (obs_log_var,)   bernoulli (link 0 / 1,)   poisson ()   studentt (log_scale, df, studentt_lognorm(df))
# ------------------------------------------------------------------------------------------------
def reg_target(y, C, B):
    """A regression / count target as the Gaussian, Poisson and Student-t kernels read it: (fp32 contiguous tensor, row stride
    ldy) -- (C, B) -> ldy = B, (B,) -> ldy = 0 (one row shared by every output: the reference's y.unsqueeze(0).unsqueeze(-1)
    broadcast).  Values are not checked."""
    if not torch.is_tensor(y):
        raise TypeError(f'reg_target: a tensor is needed, got {type(y).__name__}')
    y = y.detach().to(torch.float32).contiguous()
    if tuple(y.shape) == (B,):
        return y, 0
    if tuple(y.shape) == (C, B):
        return y, B
    raise ValueError(f'reg_target: targets must have shape ({C}, {B}) or ({B},), got {tuple(y.shape)}')


gauss_target = reg_target

BERNOULLI_LINKS = {'probit': 0, 'logit': 1}


def bernoulli_link(link):
    if link not in BERNOULLI_LINKS:
        raise ValueError(f'link must be one of {sorted(BERNOULLI_LINKS)}, got {link!r}')
    return BERNOULLI_LINKS[link]


def bernoulli_target(y, C, B):
    """A classification target as the Bernoulli kernels read it -> (t, ldt, labels), exactly one of t / labels not None:
      int64 (B,)               class indices read as one-vs-rest, t[c, b] = (y[b] == c): (None, 0, y) -- no one-hot tensor
                               (a label outside [0, C) matches no output; values are not checked);
      float / bool (C, B)      per-output targets in {0, 1}: (fp32 tensor, B, None);
      float / bool (B,)        one row shared by every output: (fp32 tensor, 0, None).
    Other integer dtypes are refused (cast to int64 for class indices, to float for 0 / 1 targets)."""
    if not torch.is_tensor(y):
        raise TypeError(f'bernoulli_target: a tensor is needed, got {type(y).__name__}')
    y = y.detach()
    if y.dtype == torch.int64:
        if tuple(y.shape) != (B,):
            raise ValueError(f'bernoulli_target: int64 class indices must have shape ({B},), got {tuple(y.shape)}; '
                             'per-output 0 / 1 targets are float or bool')
        return None, 0, y.contiguous()
    if not (y.dtype.is_floating_point or y.dtype == torch.bool):
        raise TypeError(f'bernoulli_target: int64 class indices or float / bool 0 / 1 targets, got {y.dtype}')
    if tuple(y.shape) == (B,):
        return y.to(torch.float32).contiguous(), 0, None
    if tuple(y.shape) == (C, B):
        return y.to(torch.float32).contiguous(), B, None
    raise ValueError(f'bernoulli_target: targets must have shape ({C}, {B}) or ({B},), got {tuple(y.shape)}')


def studentt_lognorm(df):
    """lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi) / 2 in double on the host: the two lgamma cancel in fp32 at large nu."""
    df = float(df)
    if not df > 0.0:
        raise ValueError(f'Student-t degrees of freedom must be > 0, got {df!r}')
    return math.lgamma(0.5 * (df + 1.0)) - math.lgamma(0.5 * df) - 0.5 * math.log(df * math.pi)


# kind -> (target function, do the nll entries take a workspace, does nll_bwd write a parameter gradient)
_LIK = {'gauss': (reg_target, False, True), 'bernoulli': (bernoulli_target, True, False),
        'poisson': (reg_target, True, False), 'studentt': (reg_target, True, True)}


def lik_target(kind, y, C, B):
    return _LIK[kind][0](y, C, B)


def _lik_call(kind, entry, mu, var, target, extra, outs, ws=None):
    """vargp_<kind>_<entry>(mu, var, *target, *extra, *outs, S, C, B, [ws, ws_bytes], stream).  Tensors and None go as pointers,
    host scalars as they are.  ws: None -- the entry takes no workspace; False -- it gets a null one; True -- pooled scratch."""
    S, C, B = mu.shape
    tail = ()
    if ws is not None:
        buf = scratch(getattr(lib(), f'vargp_{kind}_workspace_bytes')(S, C, B), mu.device) if ws else None
        tail = (ptr(buf), buf.numel() * 4 if ws else 0)
    name = f'vargp_{kind}_{entry}'
    args = [ptr(a) if a is None or torch.is_tensor(a) else a for a in (mu, var, *target, *extra, *outs)]
    check(getattr(lib(), name)(*args, S, C, B, *tail, stream_ptr()), name)


def lik_nll_fwd(kind, mu, var, target, extra, out):
    """Writes the nll of mu, var (S, C, B) fp32 contiguous into the one-float device tensor `out`."""
    _lik_call(kind, 'nll_fwd', mu, var, target, extra, (out,), ws=True if _LIK[kind][1] else None)


def lik_nll_bwd(kind, mu, var, target, extra, seed, gmu, gvar, gparam=None, nll=None):
    """ONE launch: the seeded gradients of the nll into gmu, gvar (S, C, B) and, for the kinds with a parameter, gparam (C,);
    with `nll`, the value too (bit-equal to the forward's).  Scratch is fetched only where the launch needs it (the value, or
    a parameter gradient): a captured training step without either sees no allocation."""
    _, has_ws, has_param = _LIK[kind]
    outs = (seed, gmu, gvar) + ((gparam,) if has_param else ()) + (nll,)
    _lik_call(kind, 'nll_bwd', mu, var, target, extra, outs, ws=(nll is not None or has_param) if has_ws else None)


class _LikNll(Function):
    @staticmethod
    def forward(ctx, kind, mu, var, y, param, *consts):
        require_device(mu, var, y, param)
        mu, var = mu.contiguous(), var.contiguous()
        S, C, B = mu.shape
        assert var.shape == mu.shape and mu.dtype == torch.float32 and var.dtype == torch.float32, (mu.shape, var.shape, mu.dtype, var.dtype)
        if param is not None:
            param = param.contiguous()
            assert param.shape == (C,) and param.dtype == torch.float32, (mu.shape, param.shape, param.dtype)
        target = lik_target(kind, y, C, B)
        extra = (() if param is None else (param,)) + consts
        nll = torch.empty((), dtype=torch.float32, device=mu.device)
        lik_nll_fwd(kind, mu, var, target, extra, nll)
        ctx.save_for_backward(mu, var, param)
        ctx.kind, ctx.target, ctx.consts = kind, target, consts
        return nll

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        mu, var, param = ctx.saved_tensors
        gmu, gvar = torch.empty_like(mu), torch.empty_like(var)
        gparam = torch.empty_like(param) if _LIK[ctx.kind][2] else None
        extra = (() if param is None else (param,)) + ctx.consts
        lik_nll_bwd(ctx.kind, mu, var, ctx.target, extra, g.float().contiguous(), gmu, gvar, gparam)
        return (None, gmu, gvar, None, gparam) + (None,) * len(ctx.consts)


def lik_nll(kind, mu, var, y, param, *consts):
    """The nll of mu, var (S, C, B) under the likelihood `kind`; y as its *_target takes it; param: the output's own parameter
    (C,) or None; consts: the host constants behind it in `extra`.  Differentiable in mu, var and param."""
    return _LikNll.apply(kind, mu, var, y, param, *consts)


def gauss_nll(mu, var, y, obs_log_var):
    """sum_b mean_{s,c} -log N(y | mu, var + exp(obs_log_var[c]))  (GaussianLikelihood.loss, likelihoods.py:92-107);
    y (C, B) or (B,).  Differentiable in mu, var and obs_log_var."""
    return lik_nll('gauss', mu, var, y, obs_log_var)


def bernoulli_nll(mu, var, y, link='probit'):
    """- sum_b sum_c mean_s E_{f ~ N(mu, var)} log Lambda((2 t - 1) f) by the 20-node Gauss-Hermite rule
    (BernoulliLikelihood.loss); y as bernoulli_target takes it.  Differentiable in mu and var."""
    return lik_nll('bernoulli', mu, var, y, None, bernoulli_link(link))


def poisson_nll(mu, var, y):
    """- sum_b sum_c mean_s [y mu - exp(mu + var / 2) - lgamma(y + 1)]  (PoissonLikelihood.loss); y (C, B) or (B,), non-negative.
    Differentiable in mu and var."""
    return lik_nll('poisson', mu, var, y, None)


def studentt_nll(mu, var, y, log_scale, df=4.0):
    """- sum_b sum_c mean_s E_{f ~ N(mu, var)} log t_df((y - f) / exp(log_scale[c])) / exp(log_scale[c]) by the 20-node
    Gauss-Hermite rule (StudentTLikelihood.loss); y (C, B) or (B,).  Differentiable in mu, var and log_scale."""
    return lik_nll('studentt', mu, var, y, log_scale, float(df), studentt_lognorm(df))


def bernoulli_predict(mu, var, link='probit'):
    """probs (B, C) = mean_s P(t = 1) of mu, var (S, C, B); not normalised over the outputs."""
    require_device(mu, var)
    mu, var = mu.contiguous(), var.contiguous()
    S, C, B = mu.shape
    probs = torch.empty(B, C, dtype=torch.float32, device=mu.device)
    check(lib().vargp_bernoulli_predict(ptr(mu), ptr(var), bernoulli_link(link), ptr(probs), S, C, B, stream_ptr()),
          'vargp_bernoulli_predict')
    return probs


def poisson_predict(mu, var):
    """rate (S, C, B) = E exp(f) = exp(mu + var / 2)."""
    require_device(mu, var)
    mu, var = mu.contiguous(), var.contiguous()
    S, C, B = mu.shape
    rate = torch.empty_like(mu)
    check(lib().vargp_poisson_predict(ptr(mu), ptr(var), ptr(rate), S, C, B, stream_ptr()), 'vargp_poisson_predict')
    return rate


def _lpd_moments(mu, var, *others):
    """The moments as the LPD kernels read them: fp32, contiguous, (S, C, B) each, on the device like every other operand."""
    require_device(mu, var, *others)
    mu, var = mu.detach().contiguous(), var.detach().contiguous()
    assert mu.dim() == 3 and var.shape == mu.shape and mu.dtype == torch.float32 and var.dtype == torch.float32, \
        (mu.shape, var.shape, mu.dtype, var.dtype)
    return mu, var


def softmax_lpd(mu, var, eps, y):
    """lpd (B,) = logsumexp_{s,f} log_softmax_c(mu + sqrt(var) eps)[y_b] - log(S F): the log of the mean probability of the
    label over the S F samples.  mu, var (S, C, B), eps (S, F, C, B), y int64 (B,) (not checked)."""
    mu, var = _lpd_moments(mu, var, eps, y)
    eps, y = eps.detach().contiguous(), y.detach().contiguous()
    assert y.dtype == torch.int64 and eps.dtype == torch.float32
    S, F, C, B = eps.shape
    assert mu.shape == (S, C, B) and y.shape == (B,), (mu.shape, eps.shape, y.shape)
    lpd = torch.empty(B, dtype=torch.float32, device=mu.device)
    check(lib().vargp_softmax_lpd(ptr(mu), ptr(var), ptr(eps), ptr(y), ptr(lpd), S, F, C, B, stream_ptr()), 'vargp_softmax_lpd')
    return lpd


def lik_lpd(kind, mu, var, y, extra, per_output=False):
    """lpd (B,) = logsumexp_s sum_c lp[s, c, b] - log S, the joint density of a point's targets under the mixture over
    hyper-samples (lp: the log marginal likelihood of one target under f ~ N(mu, var)); per_output: (lpd, lpd_out (C, B)) with
    lpd_out = logsumexp_s lp[s, c, b] - log S.  y as the kind's *_target takes it; a tensor in `extra` is the parameter (C,)."""
    mu, var = _lpd_moments(mu, var, y, *(a for a in extra if torch.is_tensor(a)))
    S, C, B = mu.shape
    extra = tuple(a.detach().to(torch.float32).contiguous() if torch.is_tensor(a) else a for a in extra)
    assert all(a.shape == (C,) for a in extra if torch.is_tensor(a)), (mu.shape, extra)
    lpd = torch.empty(B, dtype=torch.float32, device=mu.device)
    out = torch.empty(C, B, dtype=torch.float32, device=mu.device) if per_output else None
    _lik_call(kind, 'lpd', mu, var, lik_target(kind, y, C, B), extra, (lpd, out))
    return (lpd, out) if per_output else lpd


def gauss_lpd(mu, var, y, obs_log_var, per_output=False):
    """lik_lpd with lp = log N(y | mu, var + exp(obs_log_var[c])); y as gauss_target takes it."""
    return lik_lpd('gauss', mu, var, y, (obs_log_var,), per_output)


def bernoulli_lpd(mu, var, y, link='probit', per_output=False):
    """lik_lpd with lp = log Phi(s mu / sqrt(1 + var)) (probit, closed form; -inf below z ~ -37, where fp64 erfc underflows) or
    the 20-node rule on the logistic function (logit); y as bernoulli_target takes it."""
    return lik_lpd('bernoulli', mu, var, y, (bernoulli_link(link),), per_output)


def poisson_lpd(mu, var, y, per_output=False):
    """lik_lpd with lp = logsumexp_k(log w_k + y f_k - exp(f_k) - lgamma(y + 1)) on the 20-node rule; y as reg_target takes it."""
    return lik_lpd('poisson', mu, var, y, (), per_output)


def studentt_lpd(mu, var, y, log_scale, df=4.0, per_output=False):
    """lik_lpd with lp = logsumexp_k(log w_k + K_c - (df + 1) / 2 log1p((y - f_k)^2 / (df sigma_c^2))) on the 20-node rule; y as
    reg_target takes it, log_scale (C,)."""
    return lik_lpd('studentt', mu, var, y, (log_scale, float(df), studentt_lognorm(df)), per_output)


def _unc_moments(mu, var, *others):
    """_lpd_moments with the shape and dtype asserted BEFORE the device: a malformed call fails the same way on any tensor."""
    assert mu.dim() == 3 and var.shape == mu.shape and mu.dtype == torch.float32 and var.dtype == torch.float32, \
        (mu.shape, var.shape, mu.dtype, var.dtype)
    assert all(d > 0 for d in mu.shape), mu.shape
    return _lpd_moments(mu, var, *others)


def softmax_uncertainty(mu, var, eps):
    """The predictive entropy of the softmax and its two parts (csrc/uncertainty.hip; nats, no autograd): mu, var (S, C, B),
    eps (S, F, C, B)  ->  probs (B, C) = mean_{s,f} softmax_c(mu + sqrt(var) eps), the definition of softmax_predict;
    total (B,) = the entropy of probs; expected (B,) = the mean entropy of the S F samples; mi (B,) = max(total - expected, 0),
    subtracted in fp64 before rounding.  The (S, F, C, B) probabilities are never stored (pooled scratch: (S F + 1) B doubles)."""
    assert eps.dim() == 4 and eps.dtype == torch.float32, (eps.shape, eps.dtype)
    S, F, C, B = eps.shape
    assert tuple(mu.shape) == (S, C, B), (mu.shape, eps.shape)
    mu, var = _unc_moments(mu, var, eps)
    eps = eps.detach().contiguous()
    probs = torch.empty(B, C, dtype=torch.float32, device=mu.device)
    total, expected, mi = (torch.empty(B, dtype=torch.float32, device=mu.device) for _ in range(3))
    ws = scratch(lib().vargp_softmax_uncertainty_workspace_bytes(S, F, C, B), mu.device)
    check(lib().vargp_softmax_uncertainty(ptr(mu), ptr(var), ptr(eps), ptr(probs), ptr(total), ptr(expected), ptr(mi), S, F, C, B,
                                          ptr(ws), ws.numel() * 4, stream_ptr()), 'vargp_softmax_uncertainty')
    return probs, total, expected, mi


def bernoulli_uncertainty(mu, var, link='probit', per_output=False):
    """The predictive entropy of independent Bernoulli outputs and its two parts (csrc/uncertainty.hip; nats, no autograd), on the
    20-node Gauss-Hermite rule for either link: mu, var (S, C, B)  ->  probs (B, C) = mean_s sum_k w_k Lambda(f_k);
    total, expected, mi (B,), the sums over the outputs of h(p_out), mean_s sum_k w_k h(Lambda(f_k)) and max of their difference
    and 0; per_output: also total_out, expected_out, mi_out (C, B).  For the probit link probs differs from bernoulli_predict
    (closed form) by the rule's quadrature error."""
    link = bernoulli_link(link)
    mu, var = _unc_moments(mu, var)
    S, C, B = mu.shape
    probs = torch.empty(B, C, dtype=torch.float32, device=mu.device)
    total, expected, mi = (torch.empty(B, dtype=torch.float32, device=mu.device) for _ in range(3))
    outs = tuple(torch.empty(C, B, dtype=torch.float32, device=mu.device) for _ in range(3)) if per_output else (None,) * 3
    check(lib().vargp_bernoulli_uncertainty(ptr(mu), ptr(var), link, ptr(probs), ptr(total), ptr(expected), ptr(mi),
                                            *(ptr(o) for o in outs), S, C, B, stream_ptr()), 'vargp_bernoulli_uncertainty')
    return (probs, total, expected, mi) + (outs if per_output else ())


# ------------------------------------------------------------------------------------------------
# variational hyper-parameters
# ------------------------------------------------------------------------------------------------
class _HyperSample(Function):
    @staticmethod
    def forward(ctx, mean, logvar, eps):
        require_device(mean, logvar, eps)
        mean, logvar, eps = mean.contiguous(), logvar.contiguous(), eps.contiguous()
        S, D1 = eps.shape
        theta = torch.empty_like(eps)
        check(lib().vargp_hyper_sample_fwd(ptr(mean), ptr(logvar), ptr(eps), ptr(theta), S, D1, stream_ptr()),
              'vargp_hyper_sample_fwd')
        ctx.save_for_backward(logvar, eps)
        return theta

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        logvar, eps = ctx.saved_tensors
        S, D1 = eps.shape
        gm, gv = torch.empty_like(logvar), torch.empty_like(logvar)
        check(lib().vargp_hyper_sample_bwd(ptr(logvar), ptr(eps), ptr(g.contiguous()), ptr(gm), ptr(gv), S, D1,
                                           stream_ptr()), 'vargp_hyper_sample_bwd')
        return gm, gv, None


def hyper_sample(mean, logvar, eps):
    return _HyperSample.apply(mean, logvar, eps)


class _HyperKl(Function):
    @staticmethod
    def forward(ctx, mean, logvar, pmean, plogvar):
        require_device(mean, logvar, pmean, plogvar)
        t = [x.contiguous() for x in (mean, logvar, pmean, plogvar)]
        kl = torch.empty((), dtype=torch.float32, device=mean.device)
        check(lib().vargp_hyper_kl_fwd(*(ptr(x) for x in t), ptr(kl), mean.numel(), stream_ptr()), 'vargp_hyper_kl_fwd')
        ctx.save_for_backward(*t)
        return kl

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        t = ctx.saved_tensors
        gm, gv = torch.empty_like(t[0]), torch.empty_like(t[1])
        check(lib().vargp_hyper_kl_bwd(*(ptr(x) for x in t), ptr(g.contiguous()), ptr(gm), ptr(gv), t[0].numel(),
                                       stream_ptr()), 'vargp_hyper_kl_bwd')
        return gm, gv, None, None


def hyper_kl(mean, logvar, prior_mean, prior_logvar):
    return _HyperKl.apply(mean, logvar, prior_mean, prior_logvar)


# ------------------------------------------------------------------------------------------------
# deep-kernel feature map: Linear (+ ReLU) on the MFMA GEMM with a fused bias / activation pass
# ------------------------------------------------------------------------------------------------
class _LinearAct(Function):
    @staticmethod
    def forward(ctx, x, weight, bias, relu):
        require_device(x, weight, bias)
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        h = bgemm(x2, weight.mT)                                   # (rows, out)
        y = torch.empty_like(h)
        check(lib().vargp_bias_act_fwd(ptr(h), ptr(bias.contiguous()), ptr(y), h.shape[0], h.shape[1], int(relu),
                                       stream_ptr()), 'vargp_bias_act_fwd')
        ctx.save_for_backward(x2, weight, y)
        ctx.relu, ctx.xshape = bool(relu), x.shape
        return y.reshape(*x.shape[:-1], weight.shape[0])

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x2, weight, y = ctx.saved_tensors
        gy2 = gy.reshape(-1, weight.shape[0]).contiguous()
        gh = torch.empty_like(gy2)
        gb = torch.empty(weight.shape[0], dtype=torch.float32, device=gy.device)
        check(lib().vargp_bias_act_bwd(ptr(y), ptr(gy2), ptr(gh), ptr(gb), gy2.shape[0], gy2.shape[1], int(ctx.relu),
                                       stream_ptr()), 'vargp_bias_act_bwd')
        gx = bgemm(gh, weight).reshape(ctx.xshape) if ctx.needs_input_grad[0] else None
        gw = bgemm(gh.mT, x2) if ctx.needs_input_grad[1] else None
        return gx, gw, gb, None


def linear_act(x, weight, bias, relu):
    """act(x @ weight^T + bias) over the last dim of x; weight (out, in) as torch.nn.Linear stores it."""
    return _LinearAct.apply(x, weight, bias, relu)


# ------------------------------------------------------------------------------------------------
# triangular solve against a factor that came with its inverse (an op of its own in SURVEY §8b's list)
# ------------------------------------------------------------------------------------------------
class _TrsmLower(Function):
    @staticmethod
    def forward(ctx, L, T, B):
        require_device(L, T, B)
        T, B = T.contiguous(), B.contiguous()
        n, nrhs = B.shape[-2:]
        nb = B.numel() // (n * nrhs)
        assert T.shape[-1] == n and T.numel() == nb * n * n, 'trsm_lower: one factor per right-hand side block'
        X = torch.empty_like(B)
        check(lib().vargp_trsm_lower_fwd(ptr(T), ptr(B), ptr(X), nb, n, nrhs, stream_ptr()), 'vargp_trsm_lower_fwd')
        ctx.save_for_backward(T, X)
        return X

    @staticmethod
    @once_differentiable
    def backward(ctx, gX):
        T, X = ctx.saved_tensors
        n, nrhs = X.shape[-2:]
        nb = X.numel() // (n * nrhs)
        gB = torch.empty_like(X)
        gL = torch.empty_like(T) if ctx.needs_input_grad[0] else None
        check(lib().vargp_trsm_lower_bwd(ptr(T), ptr(X), ptr(gX.contiguous()), ptr(gB), ptr(gL), nb, n, nrhs, None, 0,
                                         stream_ptr()), 'vargp_trsm_lower_bwd')
        return gL, None, gB


def trsm_lower(L, T, B):
    """X = L^-1 B for a factor L that came with T = L^-1 from chol_inv (gradients flow to L and B; T is L's inverse,
    not an independent input)."""
    return _TrsmLower.apply(L, T, B)
