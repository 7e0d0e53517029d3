"""The ELBO through the native programs: `vargp_elbo_t0_fwd / _bwd` (csrc/elbo_t0.hip, first task) and
`vargp_elbo_tn_fwd / _bwd` (csrc/elbo_tn.hip, the block-structured program: models with previous tasks and any
forward-only evaluation).

`VARGP.loss` of a model without previous tasks (reference: var_gp/vargp.py:156-194) is, on this path, two C-ABI
calls: the forward sequences ~10 kernels (hyper-parameter sampling + KL, both kernel matrices in one GEMM launch,
one batched Cholesky/inverse, one GEMM for everything multiplied by Lz^-1, predictive moments, KL, softmax
likelihood), the backward ~20.  This module holds
  * `T0Program` / `TnProgram` — descriptor + workspace for one problem shape; `forward()` / `backward()` are the two
    calls.  Everything the two share (operand binding, the Cholesky-status protocol, backward, re-evaluation) is written
    once in `_Program`; a subclass names its C entry points and adds the operands only it has;
  * `_claim` / `_verify` / `_release` — who owns a program's workspace between a forward and its backward;
  * `elbo_node()` — a program as ONE autograd node (softmax or an external likelihood), which is what `VARGP.loss` returns
    into the reference's training loop (`loss.backward()`, experiments/vargp.py:34-35) when the lazy route is off;
  * `elbo_lazy()` — the same without an autograd graph (lazy.py), the default.
`train.ElboTrainer` drives a persistent program directly (no autograd graph, gradients written straight into the
optimiser's buffers).
"""
import ctypes
import weakref

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops
from ._lib import ElboT0Desc, ElboTnDesc, HyperGradDesc, check, lib, ptr, require_device, stream_ptr, workspace
from .ops import JITTER


def _p(t):
    return t.data_ptr() if t is not None else None


def _flat_views(shapes, device):
    """One tensor per shape as views of ONE allocation (each starting on a 256-byte boundary): one allocator call."""
    ns = [torch.Size(sh).numel() for sh in shapes]
    offs, tot = [], 0
    for n in ns:
        offs.append(tot)
        tot += (n + 63) // 64 * 64
    flat = torch.empty(tot, dtype=torch.float32, device=device)
    return [flat[o:o + n].view(sh) for o, n, sh in zip(offs, ns, shapes)]


class _Program:
    """Descriptor + workspace of one native ELBO program for a fixed shape (S, C, M, D, B, F[, nblk]).  The workspace
    carries every intermediate from `forward` to `backward`.  Subclasses: `_Desc` (the descriptor type), `_C` (the C entry
    points: ws, fwd, bwd, lik_buffers, hyper_desc), `_one_backward`."""
    _one_backward = False      # does `backward` refuse a second call on the same forward?  (T0Program only)

    def __init__(self, shape, n_info, device, map_est, ws='ws', **fields):
        S, C, M, D, B, F = shape[:6]
        self.shape = tuple(shape)
        self.map_est = bool(map_est)
        self._fn = {entry: getattr(lib(), name) for entry, name in self._C.items()}
        self.ws = workspace(self._fn[ws](*shape), device)
        self.scalars = torch.empty(3, dtype=torch.float32, device=device)
        self.info = torch.empty(n_info, dtype=torch.int32, device=device)
        self.desc = self._Desc(S=S, C=C, M=M, D=D, B=B, F=F, map_est=int(self.map_est), jitter=JITTER,
                               scalars=_p(self.scalars), info=_p(self.info), ws=_p(self.ws),
                               ws_bytes=self.ws.numel() * 4, **fields)
        self._ref = ctypes.byref(self.desc)
        self._keep = None
        self._rng = None
        self._bwd_ok = False
        # busy / _gen: a forward whose backward can still come owns the workspace (_claim below); VARGP._t0_program /
        # _tn_program then hand out a spare of the same shape
        self.busy = False
        self._gen = 0

    @staticmethod
    def shape_of(n_v, z, x, n_f):
        return (n_v, z.shape[0], z.shape[1], z.shape[2], x.shape[0], n_f)

    def _call(self, entry, *args, what=None):
        check(self._fn[entry](self._ref, *args), what or self._C[entry])

    def set_rng(self, seed, counter, sample_offset=0):
        """Native noise: `forward(eps_theta=None, eps_f=None)` then draws both noise tensors inside the program from a
        Philox4x32-10 generator keyed by `seed`; `counter` (device int32/uint32 tensor of one element) is the step
        number, advanced by every forward; `sample_offset` = index of this rank's first hyper-sample in the global
        draw (sample-parallel ranks: rank * S)."""
        assert counter.is_cuda and counter.numel() == 1 and counter.element_size() == 4
        self._rng = (int(seed), counter, int(sample_offset))
        self.desc.rng_seed, self.desc.rng_counter, self.desc.rng_sample_offset = int(seed), _p(counter), int(sample_offset)

    # -- views into the workspace ----------------------------------------------------------------------------------------------
    def _view(self, index, shape):
        # workspace layout (carve_t0 / carve_tn): theta | eps_theta | eps_f | ..., each rounded up to 64 floats
        S, C, M, D, B, F_ = self.shape[:6]
        sizes = [S * (D + 1), S * (D + 1), S * F_ * C * B]
        off = sum((n + 63) // 64 * 64 for n in sizes[:index])
        return self.ws[off:off + sizes[index]].view(shape)

    def theta(self):
        """The hyper-parameter samples of the last forward, (S, D+1)."""
        return self._view(0, (self.shape[0], self.shape[3] + 1))

    def eps_theta(self):
        """Hyper-parameter noise drawn by the last native-noise forward, (S, D+1)."""
        return self._view(1, (self.shape[0], self.shape[3] + 1))

    def eps_f(self):
        """Likelihood noise drawn by the last native-noise forward, (S, F, C, B)."""
        S, C, M, D, B, F_ = self.shape[:6]
        return self._view(2, (S, F_, C, B))

    def _ws_views(self, ptrs, B):
        """Workspace addresses handed back by the library -> (S, C, B) views."""
        S, C = self.shape[:2]
        offs = [(q.value - self.ws.data_ptr()) // 4 for q in ptrs]
        return tuple(self.ws[o:o + S * C * B].view(S, C, B) for o in offs)

    def lik_buffers(self):
        """(mu, var, gmu, gvar), each (S, C, B): the predictive moments of the last forward and the likelihood-gradient buffers
        the backward reads (views into the workspace).  With `forward(ext_lik=True)` the caller fills gmu / gvar (seeded)."""
        ps = [ctypes.c_void_p() for _ in range(4)]
        self._call('lik_buffers', *(ctypes.byref(q) for q in ps), what='lik_buffers')
        return self._ws_views(ps, self.shape[4])

    # -- the calls -------------------------------------------------------------------------------------------------------------
    def _contiguous(self, what, *tensors):
        require_device(*tensors)
        for t in tensors:
            if t is not None and not t.is_contiguous():
                raise ValueError(f'{type(self).__name__}.{what} needs contiguous tensors')

    def _bind(self, operands, x, y, eps_theta, eps_f, bump=None, **more):
        """Operand pointers into the descriptor.  operands = (log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean,
        u_tril_vec); more: the block program's z_all / rk_all.  The descriptor holds raw pointers: `_keep` keeps the tensors
        alive until the backward."""
        d = self.desc
        log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec = operands
        d.log_mean, d.log_logvar = _p(log_mean), _p(log_logvar)
        d.prior_log_mean, d.prior_log_logvar = _p(prior_log_mean), _p(prior_log_logvar)
        d.z, d.u_mean, d.u_tril_vec, d.x, d.y = _p(z), _p(u_mean), _p(u_tril_vec), _p(x), _p(y)
        d.eps_theta, d.eps_f, d.bump = _p(eps_theta), _p(eps_f), _p(bump)
        for name, t in more.items():
            setattr(d, name, _p(t))
        self._keep = (*operands, x, y, eps_theta, eps_f, bump, *more.values())

    def _forward(self, operands, x, y, eps_theta, eps_f, bump, ext_lik, lik=True, **more):
        """What the two programs' `forward` share: checks, binding, the launch with the Cholesky status words."""
        self._contiguous('forward', *operands, *more.values(), x, y, eps_theta, eps_f)
        log_mean, log_logvar, _, _, z, u_mean, u_tril_vec = operands
        S, C, M, D, B, F_ = self.shape[:6]
        assert z.shape == (C, M, D) and x.shape == (B, D)
        assert u_mean.numel() == C * M and u_tril_vec.shape == (C, M * (M + 1) // 2) and log_mean.numel() == D + 1
        if ext_lik:
            assert self.map_est or eps_theta.shape == (S, D + 1)
        elif lik and eps_f is None:
            assert self._rng is not None and eps_theta is None, 'native noise: call set_rng() and pass no eps tensors'
        elif lik:
            assert eps_f.shape == (S, F_, C, B) and (self.map_est or eps_theta.shape == (S, D + 1))
        self._bind(operands, x, y, eps_theta, eps_f, bump, **more)
        d = self.desc
        d.scalars = _p(self.scalars)                  # (VARGP.loss hands out a fresh slot of a small ring per forward: elbo_lazy)
        d.ext_lik = int(bool(ext_lik))
        self._ver = tuple(t._version for t in (log_mean, log_logvar, z, u_mean, u_tril_vec))
        # 'raise' mode: the status words are copied out and an event recorded right behind the factorisation launch (the second of
        # four): the host waits for that, and the rest of the forward runs while it carries on (combine, the backward's launch)
        # ('lazy': the same copy + event, looked at by a later call -- no torch launch for the status words at all)
        early = ops._chol_mode in ('raise', 'lazy') and not torch.cuda.is_current_stream_capturing()
        if early:
            host, ev = ops.raise_slot(self.info.numel()) if ops._chol_mode == 'raise' else ops.lazy_slot(self.info.numel())
            d.info_host, d.info_event = host.data_ptr(), ev.cuda_event
        else:
            d.info_host, d.info_event = None, None
        self._call('fwd', stream_ptr())
        self._bwd_ok = True
        if not early:
            ops._note_chol_errors(self.info)
        elif ops._chol_mode == 'raise':
            ops.raise_wait(host, ev)
        else:
            ops._pending.append((host, ev))
        return self.scalars

    def backward(self, seeds, g_log_mean, g_log_logvar, g_z, g_u_mean, g_u_tril_vec, defer_hyper=False):
        """seeds (3,) device = d total / d (kl_hypers, kl_u, nll); overwrites the five gradient buffers.
        defer_hyper: the last kernel (theta-gradient -> log_mean / log_logvar) is left to the optimiser's launch
        (`hyper_desc()` -> optim.Yogi.step(hyper=...)); g_log_mean / g_log_logvar are then written by that launch."""
        grads = (g_log_mean, g_log_logvar, g_z, g_u_mean, g_u_tril_vec)
        require_device(seeds, *grads)
        assert self._keep is not None or self._one_backward, f'{type(self).__name__}.backward without a forward'
        # (the forward clears the accumulators the backward adds into: include/vargp_hip.h, vargp_elbo_t0_bwd)
        if self._one_backward and not self._bwd_ok:
            raise RuntimeError(f'{type(self).__name__}.backward: one backward per forward (the forward clears the accumulators '
                               'the backward adds into); call rerun_forward() first to evaluate the same forward again for '
                               'another backward')
        self._bwd_ok = False
        for g in grads:
            assert g.is_contiguous() and g.dtype == torch.float32
        self.desc.defer_hyper = int(bool(defer_hyper))
        self._seeds = seeds
        self._call('bwd', ptr(seeds), ptr(g_log_mean), ptr(g_log_logvar), ptr(g_z), ptr(g_u_mean), ptr(g_u_tril_vec), stream_ptr())

    def rerun_forward(self):
        """The last forward again -- same operands, same noise, no counter advanced, status words not re-reported -- so that a
        SECOND backward can run on it (`loss.backward(retain_graph=True)` followed by another backward is legal in the
        reference's loop, experiments/vargp.py:35: ordinary autograd).  The program's backward consumes the accumulators its
        forward cleared, so the retained "graph" is re-evaluated rather than kept: results equal the first evaluation's up to the
        order of the float atomics."""
        if self._keep is None:
            raise RuntimeError('rerun_forward without a forward')
        (log_mean, log_logvar, _, _, z, u_mean, u_tril_vec) = self._keep[:7]
        if tuple(t._version for t in (log_mean, log_logvar, z, u_mean, u_tril_vec)) != self._ver:
            raise RuntimeError('one of the variables needed for gradient computation has been modified by an inplace operation '
                               '(a parameter changed between VARGP.loss and this second backward of its retained graph)')
        d = self.desc
        if not d.eps_f and not d.ext_lik:                 # the program drew the noise itself: it is still in the workspace
            et = None if self.map_est else self.eps_theta().clone()
            ef = self.eps_f().clone()
            d.eps_theta, d.eps_f = _p(et), _p(ef)
            self._keep = self._keep + (et, ef)
        if getattr(self, '_rerun_scal', None) is None:
            self._rerun_scal = torch.empty(3, dtype=torch.float32, device=self.ws.device)
        d.bump, d.info_host, d.info_event = None, None, None
        d.scalars = _p(self._rerun_scal)                  # (the first evaluation's numbers stay where the caller reads them)
        self._call('fwd', stream_ptr(), what='rerun_forward')
        self._bwd_ok = True

    def hyper_desc(self):
        """What the deferred last step of `backward(defer_hyper=True)` needs (pointers into this program's workspace)."""
        h = HyperGradDesc()
        self._call('hyper_desc', ptr(self._seeds), ctypes.byref(h))
        return h


class T0Program(_Program):
    """The native first-task ELBO (csrc/elbo_t0.hip) for fixed (S, C, M, D, B, F); one `backward` per `forward`."""
    _Desc = ElboT0Desc
    _C = dict(ws='vargp_elbo_t0_workspace_bytes', fwd='vargp_elbo_t0_fwd', bwd='vargp_elbo_t0_bwd',
              lik_buffers='vargp_elbo_t0_lik_buffers', hyper_desc='vargp_elbo_t0_hyper_desc')
    _one_backward = True

    def __init__(self, S, C, M, D, B, F, device, map_est=False):
        super().__init__((S, C, M, D, B, F), S * C + C, device, map_est)

    def forward(self, log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec, x, y, eps_theta,
                eps_f, bump=None, defer_softmax=False, ext_lik=False):
        """-> scalars (3,) = (kl_hypers, kl_u, nll).  All tensors contiguous fp32 on the ROCm device (y int64).
        ext_lik: the likelihood is the caller's (class-sharded ranks, include/vargp_hip.h): moments + KL only, nll stays 0;
        y / eps_f may be None; fill lik_buffers()[2:] before `backward`.
        defer_softmax: the caller runs `backward` right behind this forward and reads nll only afterwards (ElboTrainer): the
        likelihood is then evaluated inside the backward's tile kernel where the shapes allow (include/vargp_hip.h).
        eps_theta = eps_f = None: the program draws the noise itself (see set_rng).  `bump`: optional device float that the forward increments by one (an optimiser's step counter)."""
        assert ext_lik or y.dtype == torch.int64
        self.desc.defer_softmax = int(bool(defer_softmax))
        return self._forward((log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec), x, y, eps_theta,
                             eps_f, bump, ext_lik)


    def plan(self, cus=None):
        """The launch plan (T0Plan, csrc/elbo_t0.hip) of this program's descriptor as it stands -- after a forward: of that
        forward and its backward -- as {member: bool | int}.  cus: CU count to plan for (None: the current device's)."""
        return _plan_of(self.desc, cus)


def _plan_of(desc, cus):
    buf = ctypes.create_string_buffer(2048)
    check(lib().vargp_elbo_t0_plan(ctypes.byref(desc), int(cus or 0), buf, len(buf)), 'vargp_elbo_t0_plan')
    plan = {}
    for line in buf.value.decode().splitlines():
        name, _, value = line.partition('=')
        plan[name] = value == 'true' if value in ('true', 'false') else int(value)
    return plan


def t0_plan(S, C, M, D, B, F, cus=None, defer_softmax=False, ext_lik=False, native=False, map_est=False):
    """The launch plan the first-task program takes for these dimensions and flags (vargp_elbo_t0_plan: the library's own
    t0_plan, not a copy of its rules) as {member: bool | int}, with every operand on a 16-byte boundary.  native: the program
    draws its own noise (eps_f = NULL).  Host arithmetic: with `cus` given no device is needed."""
    aligned = 4096                                        # (only the alignment of z, x and eps_f is read)
    desc = ElboT0Desc(S=S, C=C, M=M, D=D, B=B, F=F, map_est=int(bool(map_est)), jitter=JITTER, z=aligned, x=aligned,
                      eps_f=None if native else aligned, defer_softmax=int(bool(defer_softmax)), ext_lik=int(bool(ext_lik)))
    return _plan_of(desc, cus)


def _claim(prog, owner):
    """`owner` (an autograd ctx, a lazy.PendingForward) takes the workspace of `prog` until its backward has run -- or until it
    dies without one (validation ELBO under no_grad: no graph is recorded and the ctx is released as soon as apply() returns; a
    dropped graph; a skipped step).  -> the generation to `_verify` / `_release` with."""
    prog._gen += 1
    prog.busy = True
    weakref.finalize(owner, _release, prog, prog._gen)
    return prog._gen


def _verify(prog, gen):
    if prog._gen != gen:
        raise RuntimeError(_REUSED)


def _release(prog, gen):
    if prog._gen == gen:
        prog.busy = False


_REUSED = ('VARGP.loss: the workspace of this ELBO node has been handed to a later loss() -- its forward cannot be re-evaluated '
           'for another backward.  Keep the graph with loss.backward(retain_graph=True) (the workspace then stays with this '
           'loss until it is dropped), or call loss() again')


# ----------------------------------------------------------------------------------------------------------------
# models with previous tasks (and any forward-only evaluation): the block-structured program, csrc/elbo_tn.hip
# ----------------------------------------------------------------------------------------------------------------
def tn_row_width(M):
    """Row width NR of the packed operand rk_all: [u_mean | 0 0 0 | Lu (M columns)] rounded up to a multiple of 4."""
    return (4 + M + 3) // 4 * 4


def pack_tn_operands(prev, C, M, D, device):
    """Caller-maintained operands of the program for a model whose earlier tasks are `prev` (list of dicts with z
    (C,M,D), u_mean (C,M,1), u_tril (C,M,M), all M equal): z_all (C, Mt, D) and rk_all (C, nblk, M, NR) with the earlier
    tasks filled in and the last block left for the program (it writes the current task there on every forward)."""
    nblk = len(prev) + 1
    NR = tn_row_width(M)
    z_all = torch.zeros(C, nblk * M, D, dtype=torch.float32, device=device)
    rk_all = torch.zeros(C, nblk, M, NR, dtype=torch.float32, device=device)
    for i, p in enumerate(prev):
        z_all[:, i * M:(i + 1) * M] = p['z']
        rk_all[:, i, :, 0] = p['u_mean'].reshape(C, M)
        rk_all[:, i, :, 4:4 + M] = p['u_tril']
    return z_all, rk_all


class TnProgram(_Program):
    """`vargp_elbo_tn_*` for fixed (S, C, M, D, B, F, nblk).  `forward(y=None)` evaluates the predictive moments only.
    kernel_nu2: kernels.native_code of the model's kernel (0: RBF; 1 | 3 | 5: Matern) -- a property of the program like its
    shape (`key`: what callers cache programs under, so an RBF and a Matern model of equal shape never share one)."""
    _Desc = ElboTnDesc
    _C = dict(ws='vargp_elbo_tn_workspace_bytes', ws_fwd='vargp_elbo_tn_workspace_bytes_fwd', fwd='vargp_elbo_tn_fwd',
              bwd='vargp_elbo_tn_bwd', lik_buffers='vargp_elbo_tn_lik_buffers', hyper_desc='vargp_elbo_tn_hyper_desc')

    def __init__(self, S, C, M, D, B, F, nblk, device, map_est=False, forward_only=False, kernel_nu2=0):
        # forward_only: predictive moments only (VARGP.forward / predict): none of the gradient buffers is carved
        self.forward_only = bool(forward_only)
        if kernel_nu2 not in (0, 1, 3, 5):
            raise ValueError(f'TnProgram: kernel_nu2 must be 0 (RBF) or 1, 3, 5 (Matern), got {kernel_nu2!r}')
        self.kernel_nu2 = int(kernel_nu2)
        # (the workspace does not depend on the kernel: the Matern backward recomputes d2 into buffers that are dead by then)
        super().__init__((S, C, M, D, B, F, nblk), S * C, device, map_est, ws='ws_fwd' if self.forward_only else 'ws',
                         nblk=nblk, forward_only=int(self.forward_only), kernel_nu2=self.kernel_nu2)

    @property
    def key(self):
        return self.shape + (self.kernel_nu2,)

    def moments(self, Bt=None):
        """(mu, var) (S, C, B) of the last forward (or (S, C, Bt) of the last moments-only tile): views into the workspace."""
        ps = (ctypes.c_void_p(), ctypes.c_void_p())
        check(lib().vargp_elbo_tn_moments(ctypes.byref(self.desc), *(ctypes.byref(q) for q in ps)), 'vargp_elbo_tn_moments')
        return self._ws_views(ps, self.shape[4] if Bt is None else int(Bt))

    def forward(self, log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec, z_all, rk_all, x, y,
                eps_theta, eps_f, bump=None, ext_lik=False, eps_u=None):
        """-> scalars (3,) = (kl_hypers, kl_u, nll) (y given) or None (y None: moments only).  ext_lik: as T0Program.forward
        (y must still be given: it switches the KL on).  eps_u (n_v, S, C, (nblk - 1) M): ep_var_mean = False -- the KL keeps the
        conditional prior's mean at these n_v samples of u_<t (include/vargp_hip.h: no_var_mean)."""
        S, C, M, D, B, F_, nblk = self.shape
        assert z_all.shape == (C, nblk * M, D) and rk_all.shape == (C, nblk, M, tn_row_width(M))
        assert (y is not None or not ext_lik) and (y is None or y.dtype == torch.int64)
        d = self.desc
        if eps_u is not None:
            require_device(eps_u)
            assert nblk > 1 and eps_u.is_contiguous() and eps_u.dim() == 4 and eps_u.shape[1:] == (S, C, (nblk - 1) * M), eps_u.shape
            d.n_v, d.no_var_mean = int(eps_u.shape[0]), 1
        else:
            d.n_v, d.no_var_mean = 0, 0
        scal = self._forward((log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec), x, y, eps_theta,
                             eps_f, bump, ext_lik, lik=y is not None, z_all=z_all, rk_all=rk_all, eps_u=eps_u)
        return scal if y is not None else None

    # -- predictive sweep: the x-independent part once (sweep_begin), then moments per tile of <= B points --------------------
    def sweep_begin(self, log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec, z_all, rk_all, eps_theta):
        """theta (from eps_theta (S, D+1); None under map_est), K(z_<=t), L, T and the small products: everything of the
        predictive moments that does not depend on x (vargp_elbo_tn_begin)."""
        operands = (log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec)
        self._contiguous('sweep_begin', *operands, z_all, rk_all, eps_theta)
        S, D = self.shape[0], self.shape[3]
        assert self.map_est or (eps_theta is not None and eps_theta.shape == (S, D + 1))
        # x is not read by begin (any non-null device pointer)
        self._bind(operands, z, None, eps_theta, None, z_all=z_all, rk_all=rk_all)
        check(lib().vargp_elbo_tn_begin(ctypes.byref(self.desc), stream_ptr()), 'vargp_elbo_tn_begin')
        ops._note_chol_errors(self.info)

    def sweep_moments(self, x):
        """x (Bt <= B, D) -> (mu, var) (S, C, Bt): views into the workspace, valid until the next tile."""
        S, C, M, D, B, F_, nblk = self.shape
        require_device(x)
        assert x.dim() == 2 and x.shape[1] == D and x.shape[0] <= B and x.is_contiguous()
        check(lib().vargp_elbo_tn_tile(ctypes.byref(self.desc), None, ptr(x), None, None, x.shape[0], stream_ptr()),
              'vargp_elbo_tn_tile')
        return self.moments(x.shape[0])

    # -- N-tiled ELBO: loss and gradient over a data set swept in minibatch tiles (vargp_elbo_tn_begin / _tile / _end) ----
    def tiled_step(self, log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec, z_all, rk_all, x, y,
                   seeds, grads, eps_theta=None, eps_f=None):
        """x (N, D), y (N): swept in tiles of this program's B columns (the last one may be narrower).  seeds (3,) device =
        d total / d (kl_hypers, kl_u, nll); grads = the five gradient buffers (log_mean, log_logvar, z, u_mean, u_tril_vec),
        overwritten.  eps_f (S, F, C, N) / eps_theta (S, D+1): injected noise (tests); None: native noise (set_rng).
        -> scalars (kl_hypers, kl_u, sum over the tiles of nll)."""
        B, D = self.shape[4], self.shape[3]
        operands = (log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec)
        require_device(*operands, z_all, rk_all, x, y, seeds, eps_theta, eps_f, *grads)
        assert x.dim() == 2 and x.shape[1] == D and x.is_contiguous() and y.dtype == torch.int64 and y.is_contiguous()
        if eps_f is None:
            assert self._rng is not None and (eps_theta is None), 'native noise: call set_rng() and pass no eps tensors'
        self._bind(operands, x, y, eps_theta, None, z_all=z_all, rk_all=rk_all)      # (eps_f goes in tile by tile)
        self._keep += (seeds, eps_f) + tuple(grads)
        d, st = self.desc, stream_ptr()
        check(lib().vargp_elbo_tn_begin(ctypes.byref(d), st), 'vargp_elbo_tn_begin')
        N = x.shape[0]
        for i in range(0, N, B):
            bt = min(B, N - i)
            ef = None if eps_f is None else eps_f[..., i:i + bt].contiguous()
            check(lib().vargp_elbo_tn_tile(ctypes.byref(d), ptr(seeds), ptr(x[i:i + bt]), ptr(y[i:i + bt]), ptr(ef), bt, st),
                  'vargp_elbo_tn_tile')
        check(lib().vargp_elbo_tn_end(ctypes.byref(d), ptr(seeds), *(ptr(g) for g in grads), st), 'vargp_elbo_tn_end')
        ops._note_chol_errors(self.info)
        return self.scalars


# ----------------------------------------------------------------------------------------------------------------
# External likelihoods (likelihoods.is_external: GaussianLikelihood -- regression, var_gp/likelihoods.py:66-110 --,
# BernoulliLikelihood, PoissonLikelihood, StudentTLikelihood) on either program: the program's forward with ext_lik stops
# at the predictive moments and the KL, the likelihood's value and its seeded gradients are one call each
# (likelihood.ext_value / ext_backward over lik_views(prog): csrc/gauss_lik.hip, csrc/indep_lik.hip),
# and the program's backward takes those gradients from its likelihood buffers
# ----------------------------------------------------------------------------------------------------------------
_Y_DUMMY = {}


def y_dummy(device):
    """The block program needs a non-NULL label pointer to evaluate the KL under ext_lik; it never reads it."""
    dev = torch.device(device)
    t = _Y_DUMMY.get(dev)
    if t is None:
        t = _Y_DUMMY[dev] = torch.zeros(1, dtype=torch.int64, device=dev)
    return t


def lik_views(prog):
    """prog.lik_buffers(), looked up once per program (the views stay valid for the program's lifetime)."""
    v = getattr(prog, '_lik_views', None)
    if v is None:
        v = prog._lik_views = prog.lik_buffers()
    return v


# ----------------------------------------------------------------------------------------------------------------
# VARGP.loss on a native program as ONE autograd node
# ----------------------------------------------------------------------------------------------------------------
class _Elbo(Function):
    """Differentiable inputs: the program's operands (VARGP._operands order; the two prior tensors get no gradient) and an
    external likelihood's own parameter (lik.ext_param(): GaussianLikelihood's obs_log_var; None otherwise).  lik: the
    external likelihood (None: the softmax likelihood inside the program).  `packed` = (z_all, rk_all) on the block program,
    () on the first-task program."""

    @staticmethod
    def forward(ctx, log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec, lik_param, x, y,
                eps_theta, eps_f, map_est, prog, packed, eps_u, lik):
        c = lambda t: None if t is None else t.contiguous()
        ext = lik is not None
        if prog is None:         # no cached program handed in: a workspace of this node's own
            S = 1 if map_est else eps_theta.shape[0]
            prog = T0Program(*T0Program.shape_of(S, z, x, eps_f.shape[1]), z.device, map_est)
        labels = c(y) if not ext else y_dummy(x.device) if packed else None
        prog.forward(*map(c, (log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean, u_tril_vec)), *packed,
                     c(x), labels, c(eps_theta), c(eps_f), ext_lik=ext, **(dict(eps_u=c(eps_u)) if packed else {}))
        if ext:                  # the likelihood's value between the program's forward and backward
            ctx.target = lik.ext_target(y, z.shape[0], x.shape[0])
            lik.ext_value(prog, ctx.target)
        scal = prog.scalars.clone()          # the program's scalars are overwritten by its next forward
        # grad mode is always off inside Function.forward, so the node's lifetime is the signal for ownership
        ctx.gen = _claim(prog, ctx)
        ctx.prog, ctx.map_est, ctx.lik = prog, map_est, lik
        ctx.shapes = (log_mean.shape, log_mean.shape, z.shape, u_mean.shape, u_tril_vec.shape)
        return scal[0], scal[1], scal[2]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_klh, g_klu, g_nll):
        prog = ctx.prog
        _verify(prog, ctx.gen)
        if getattr(ctx, 'ran', False):
            prog.rerun_forward()             # second backward of a retained graph: the forward is evaluated again
        ctx.ran = True
        seeds = torch.stack([g_klh.reshape(()), g_klu.reshape(()), g_nll.reshape(())]).float()
        g_lik = ctx.lik.ext_backward(prog, ctx.target, seeds[2:]) if ctx.lik is not None else None
        g_mean, g_logvar, g_z, g_um, g_uv = _flat_views(ctx.shapes, seeds.device)
        prog.backward(seeds, g_mean, g_logvar, g_z, g_um, g_uv)       # (ext_lik: seeds[2] is not read)
        _release(prog, ctx.gen)              # (a later loss() may take the workspace: a further backward of THIS node then raises)
        return (g_mean, None if ctx.map_est else g_logvar, None, None, g_z, g_um, g_uv, g_lik) + (None,) * 9


def elbo_node(operands, map_est, x, y, eps_theta, eps_f, prog=None, packed=(), eps_u=None, likelihood=None):
    """-> (kl_hypers, kl_u, nll) of VARGP.loss as ONE autograd node.  operands: VARGP._operands(detach=False); `prog`: the
    (cached, not busy) program of this shape -- None: a first-task program of the node's own; packed: VARGP._tn_operands() on
    the block program; eps_u: ep_var_mean = False; likelihood: an external likelihood (GaussianLikelihood, BernoulliLikelihood;
    eps_f is then None)."""
    lik_param = likelihood.ext_param() if likelihood is not None else None
    return _Elbo.apply(*operands, lik_param, x, y, eps_theta, eps_f, bool(map_est), prog, tuple(packed), eps_u, likelihood)


# ----------------------------------------------------------------------------------------------------------------
# VARGP.loss on a native program WITHOUT an autograd graph: lazy terms (vargp_amd/lazy.py)
# ----------------------------------------------------------------------------------------------------------------
_RING = 8


def elbo_lazy(model, x, y, prog, packed=()):
    """(kl_hypers, kl_u, nll) of `model.loss(x, y)` as lazy terms over ONE forward of the model's cached program; the caller's
    linear combination and its `.backward()` become one program backward with those coefficients as seeds (lazy.py).
    Noise: injected / sharded draws if set (noise.py), otherwise the program's own counter-based generator under a key drawn
    from torch's default generator at the model's first step -- no torch.randn launches on the step."""
    from . import noise
    from .lazy import PendingForward, terms_of
    kern = model.kernel
    if getattr(prog, '_ring', None) is None:
        prog._ring, prog._ring_i = torch.zeros(_RING, 3, dtype=torch.float32, device=x.device), 0
        prog._ring_owner = [None] * _RING
    prog._ring_i = (prog._ring_i + 1) % _RING
    # the slot's previous forward, _RING steps back: if a term of it is still alive (`running += lik.detach()` read at the end
    # of the epoch, losses kept in a list), its three numbers move into a tensor of their own before the slot is reused -- a
    # term never silently reads another step's values (the copy is queued in front of this forward, same stream)
    old = prog._ring_owner[prog._ring_i]
    old = old() if old is not None else None
    if old is not None and old.values.data_ptr() == prog._ring[prog._ring_i].data_ptr():
        old.values = old.values.clone()
    prog.scalars = prog._ring[prog._ring_i]
    eps_u = model.draw_u_noise(x) if packed else None         # ep_var_mean = False only (None otherwise)
    if noise._injected or noise._shard is not None or eps_u is not None:
        eps_theta, eps_f = model.draw_t0_noise(x)
        eps_theta = None if eps_theta is None else eps_theta.contiguous()
        eps_f = eps_f.contiguous()
    else:
        if prog._rng is None:
            if getattr(model, '_noise_counter', None) is None or model._noise_counter.device != x.device:
                model._noise_counter = torch.zeros(1, dtype=torch.int32, device=x.device)
                # the stream's key is DRAWN from torch's default generator when the model takes its first step: it follows
                # torch.manual_seed like any other draw, and every model of a process (one per task in the continual-learning
                # driver, the members of an ensemble) gets a stream of its own -- keyed by torch.initial_seed() all of them
                # replayed the same noise
                model._noise_seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
            prog.set_rng(model._noise_seed, model._noise_counter)
        eps_theta = eps_f = None
    x = x if x.is_contiguous() else x.contiguous()
    y = y if y.is_contiguous() else y.contiguous()
    prog.forward(*model._operands(), *packed, x, y, eps_theta, eps_f, **(dict(eps_u=eps_u) if packed else {}))
    params = (kern.log_mean, None if kern.map_est else kern.log_logvar, model.z, model.u_mean, model.u_tril_vec)
    fwd = PendingForward(model, prog, prog.scalars, params)
    prog._ring_owner[prog._ring_i] = weakref.ref(fwd)
    return terms_of(fwd)
