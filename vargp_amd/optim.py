"""Yogi optimiser on the fused HIP step kernel (reference call site: experiments/vargp.py:23,37 uses
torch_optimizer.Yogi).

torch_optimizer is not available in this environment and is unpinned in the reference's
environment.yml, so the arithmetic follows the published algorithm (Zaheer et al., NeurIPS 2018) with
the defaults torch_optimizer documents: betas (0.9, 0.999), eps 1e-3, initial_accumulator 1e-6 for
both moment buffers.  PARITY UNPINNED for optimiser trajectories.
"""
import ctypes

import torch

from ._lib import check, lib, ptr, require_device, stream_ptr


def _dense(t):
    """Do the numel() elements of t fill one block of storage without gaps or overlap, in some order of the axes?"""
    expect = 1
    for stride, size in sorted((st, n) for n, st in zip(t.shape, t.stride()) if n != 1):
        if stride != expect:
            return False
        expect *= size
    return True


def _same_layout(a, b):
    return a.stride() == b.stride() or (a.is_contiguous() and b.is_contiguous())


class Yogi(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-2, betas=(0.9, 0.999), eps=1e-3, initial_accumulator=1e-6):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, initial_accumulator=initial_accumulator))
        # True: somebody else advances the device-side step count before step() (ElboTrainer lets the ELBO
        # program's first kernel do it), so step() launches nothing but the update kernel
        self.external_step = False
        self._chunk_cache = {}

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._chunk_cache = {}                 # the moment buffers are new tensors

    def __getstate__(self):
        # the cache holds ctypes pointer arrays (not picklable, not deep-copyable) of addresses that mean nothing elsewhere
        state = super().__getstate__() if hasattr(super(), '__getstate__') else dict(self.__dict__)
        state = dict(state)
        state.pop('_chunk_cache', None)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self._chunk_cache = {}
        self.__dict__.setdefault('external_step', False)

    def step_counter(self, device):
        """The device-side step count of the (single) parameter group."""
        group = self.param_groups[0]
        if 'step' not in group:
            group['step'] = torch.zeros(1, dtype=torch.float32, device=device)
        return group['step']

    @torch.no_grad()
    def step(self, hyper=None):
        """One fused launch for all parameter tensors of a group (<= 8).  The step count lives on the
        device (bias corrections are computed inside the kernel), so the whole step can sit inside a
        captured hipGraph.
        hyper = (HyperGradDesc, log_mean, log_logvar): the gradients of those two parameters are finished inside this
        launch (an ELBO program's backward ran with defer_hyper=True) and stored into their .grad as well."""
        for group in self.param_groups:
            b1, b2 = group['betas']
            ps = [p for p in group['params'] if p.grad is not None]
            if not ps:
                continue
            if 'step' not in group:
                group['step'] = torch.zeros(1, dtype=torch.float32, device=ps[0].device)
            if not self.external_step:
                group['step'].add_(1.0)
            for p in ps:
                st = self.state[p]
                if not st:
                    require_device(p, p.grad)
                    st['exp_avg'] = torch.full_like(p, group['initial_accumulator'])
                    st['exp_avg_sq'] = torch.full_like(p, group['initial_accumulator'])
            for i in range(0, len(ps), 8):
                chunk = ps[i:i + 8]
                k = len(chunk)
                arr = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])
                # parameters and moment buffers keep their addresses from step to step: their pointer arrays are built once
                # per chunk (the eager drop-in loop is host-bound; this call used to cost ~60 us of Python)
                key = tuple(id(p) for p in chunk)
                cached = self._chunk_cache.get(key)
                # valid while the parameters AND both moment buffers sit where they sat when the arrays were built (a moment
                # tensor replaced through optim.state, state.clear(), a move to another device: rebuilt)
                where = tuple(t.data_ptr() for p in chunk for t in (p, self.state[p]['exp_avg'], self.state[p]['exp_avg_sq']))
                if cached is None or cached[0] != where:
                    for p in chunk:
                        if not _dense(p):
                            raise ValueError(
                                f'Yogi: a parameter of shape {tuple(p.shape)} with strides {p.stride()} is not dense (a strided '
                                'slice of a larger tensor?): the fused step would update memory between its elements. Optimise '
                                'the whole tensor, or a contiguous copy of the slice.')
                        for name in ('exp_avg', 'exp_avg_sq'):
                            if not _same_layout(self.state[p][name], p):
                                raise ValueError(f'Yogi: {name} has strides {self.state[p][name].stride()}, its parameter '
                                                 f'{p.stride()}: the moment buffers must share the layout of their parameter')
                    cached = (where, arr(chunk), arr([self.state[p]['exp_avg'] for p in chunk]),
                              arr([self.state[p]['exp_avg_sq'] for p in chunk]),
                              (ctypes.c_int64 * k)(*[p.numel() for p in chunk]))
                    self._chunk_cache[key] = cached
                _, a_p, a_m, a_v, sizes = cached
                # the kernel walks p, g, m, v in STORAGE order: the gradient goes in the parameter's own layout (row-major for
                # the usual contiguous parameter; the strides of a dense transposed one -- checked where the cache is built)
                grads = [(p.grad if p.grad.is_contiguous() else p.grad.contiguous()) if p.is_contiguous() else
                         (p.grad if p.grad.stride() == p.stride() else torch.empty_like(p).copy_(p.grad)) for p in chunk]
                if not all(g.is_cuda for g in grads):
                    require_device(*grads)
                ids = list(key)
                if hyper is not None and id(hyper[1]) in ids:
                    h, p_mean, p_logvar = hyper
                    i_lv = ids.index(id(p_logvar)) if (p_logvar is not None and id(p_logvar) in ids) else -1
                    check(lib().vargp_yogi_step_multi_hyper(
                        k, a_p, arr(grads), a_m, a_v, sizes, group['lr'], b1, b2, group['eps'],
                        ptr(group['step']), 0, ctypes.byref(h), ids.index(id(p_mean)), i_lv, stream_ptr()),
                        'vargp_yogi_step_multi_hyper')
                    continue
                check(lib().vargp_yogi_step_multi(k, a_p, arr(grads), a_m, a_v, sizes,
                                                  group['lr'], b1, b2, group['eps'], ptr(group['step']), 0,
                                                  stream_ptr()),
                      'vargp_yogi_step_multi')


def choose_params(who, named, params):
    """The tensors of the non-empty subset `params` of the names of `named`, each once, in the order given; ValueError else."""
    params = tuple(params)
    if not params or any(p not in named for p in params):
        raise ValueError(f'{who}: params must be a non-empty subset of {sorted(named)}, got {params!r}')
    return [named[p] for p in dict.fromkeys(params)]


def ascend_(bound_fn, chosen, n_steps, lr):
    """n_steps steps of the project's Yogi (optim.py) up sum_c bound_fn() over the tensors `chosen`; their grads are cleared
    afterwards.  -> [the (C,) bound BEFORE each step, detached]; no synchronisation."""
    opt = Yogi(chosen, lr=lr)
    trace = []
    for _ in range(n_steps):
        bound = bound_fn()
        for p, g in zip(chosen, torch.autograd.grad(-bound.sum(), chosen)):
            p.grad = g.to(p.dtype)
        opt.step()
        trace.append(bound.detach())
    for p in chosen:
        p.grad = None
    return trace
