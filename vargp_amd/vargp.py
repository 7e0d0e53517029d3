"""VAR-GP model: API of the reference's `var_gp.vargp.VARGP` (var_gp/vargp.py:11-243) with the ELBO
hot path on the HIP kernels (see gp_utils.py / ops.py).

Differences that do not change results:
  * the minibatch is never expanded over classes (reference vargp.py:106): the kernel-matrix op takes
    the shared (B, D) block directly;
  * for tasks t > 0 the prior covariance of p(u_t | u_<t, theta) does not depend on the u_<t sample,
    so its Cholesky is computed once per (s, c) instead of n_v times (reference vargp.py:146-155), and
    with ep_var_mean=True (the default) the KL does not depend on the u_<t sample at all,
    so that sample is not drawn;
  * with ep_var_mean=True, `loss` of a model with previous tasks runs as ONE native program in the block-structured
    form of the linear_joint chain (csrc/elbo_tn.hip, fused.TnProgram): one kernel matrix over all inducing points, one
    factorisation, GEMMs; `compute_q` / `compute_pf_diag` / `forward(loss_cache=...)` below keep the reference's
    op-by-op composition (API surface, the ep_var_mean=False ablation, and what the program is tested against);
    gradient-free `forward` / `predict` use the same program for every model.
"""
import os

import torch
import torch.nn as nn

from . import collapsed, fused, gp_utils, init, loo, noise, ops, sites
from .gp_utils import vec2tril, mat2trilvec, cholesky, rev_cholesky, gp_cond, block_joint, linear_marginal_diag
from .kernels import RBFKernel, DeepRBFKernel, MaternKernel, native_code
from .likelihoods import (BernoulliLikelihood, GaussianLikelihood, MulticlassSoftmax, PoissonLikelihood, StudentTLikelihood,
                          cat_uncertainty, is_external, n_f, predict_batch_dim)
from .ops import LOWER
from .paths import PosteriorPaths


_KERNEL_NU = {'rbf': None, 'matern12': 0.5, 'matern32': 1.5, 'matern52': 2.5}   # create_clf(kernel=)


def make_clf_likelihood(likelihood, n_f, link='probit'):
    """create_clf(likelihood=, link=) -> the likelihood module; ValueError for an unknown name or link."""
    if likelihood == 'softmax':
        return MulticlassSoftmax(n_f=n_f)
    if likelihood == 'bernoulli':
        return BernoulliLikelihood(link=link)
    raise ValueError(f"create_clf: likelihood must be 'softmax' or 'bernoulli', got {likelihood!r}")


def make_reg_likelihood(likelihood, out_size, df=4.0):
    """create_reg(likelihood=, df=) -> the likelihood module; ValueError for an unknown name."""
    if likelihood == 'gaussian':
        return GaussianLikelihood(out_size)
    if likelihood == 'studentt':
        return StudentTLikelihood(out_size, df=df)
    if likelihood == 'poisson':
        return PoissonLikelihood()
    raise ValueError(f"create_reg: likelihood must be 'gaussian', 'studentt' or 'poisson', got {likelihood!r}")


def _hand_over_hyper_prior(prev_params, dkl=False):
    """The hyper-prior of the next task = the last task's hyper-posterior: popped from prev_params, which is mutated like the
    reference does (vargp.py:213-222).  dkl: the feature map starts from the last task's too (vargp.py:218-219).
    -> (prior_log_mean, prior_log_logvar, phi_params or None)"""
    if not prev_params:
        return None, None, None
    last = prev_params[-1]
    prior = last.get('kernel.log_mean'), last.get('kernel.log_logvar')
    phi_params = {k[11:]: v for k, v in last.items() if k.startswith('kernel.phi.')} if dkl else None
    for p in prev_params:
        for k in [k for k in p if k.startswith('kernel')]:
            p.pop(k)
    return (*prior, phi_params)


def _make_kernel(in_size, kernel, dkl, native_kernel, prior_log_mean, prior_log_logvar, map_est_hypers, phi_params):
    """The kernel module of a factory's (kernel=, dkl=, native_kernel=) with the handed-over hyper-prior."""
    prior = dict(prior_log_mean=prior_log_mean, prior_log_logvar=prior_log_logvar, map_est=map_est_hypers)
    if dkl:
        kern = DeepRBFKernel(in_size, **prior)
        if phi_params:
            kern.phi.load_state_dict(phi_params)
        return kern
    if kernel != 'rbf':
        return MaternKernel(in_size, nu=_KERNEL_NU[kernel], native=bool(native_kernel), **prior)
    return RBFKernel(in_size, **prior)


_Z_INITS = ('greedy', 'kmeans', 'random')                  # create_clf / create_reg (z_init=)
_LENGTHSCALE_INITS = ('default', 'median')        # (lengthscale_init=)

# q_init= of the factories.  name: ({factory that accepts it: (the likelihoods it applies to, the refusal of another) or None},
# the model checker, the fit as a function of (gp, x, y, o), o the factory's options by name).
_CLOSED_FORM = (lambda lik: lik == 'gaussian', "q_init={q!r} is the closed form of likelihood='gaussian', got {lik!r}")
_REG_SITES = (lambda lik: lik != 'gaussian', "q_init={q!r} iterates Gaussian sites of a non-Gaussian likelihood ('poisson', "
              "'studentt'); likelihood='gaussian' has the closed form q_init='optimal'")
_CLF_SITES = (lambda lik: lik == 'bernoulli', 'q_init={q!r} fits independent Gaussian sites, which likelihood={lik!r} does not have '
              "(its outputs are coupled); use likelihood='bernoulli'")
_Q_INIT = {
    'default': (dict(create_reg=None, create_clf=None), None, None),
    'optimal': (dict(create_reg=_CLOSED_FORM), collapsed.check_supported, lambda gp, x, y, o: gp.fit_q_(x, y)),
    'collapsed': (dict(create_reg=_CLOSED_FORM), collapsed.check_differentiable,
                  lambda gp, x, y, o: gp.fit_collapsed_(x, y, n_steps=o['collapsed_steps'])),
    'newton': (dict(create_reg=_REG_SITES, create_clf=_CLF_SITES), sites.check_supported,
               lambda gp, x, y, o: gp.fit_q_newton_(x, y, n_iters=o['newton_iters'], start='prior')),
    'em': (dict(create_reg=_REG_SITES, create_clf=_CLF_SITES), sites.check_differentiable,
           lambda gp, x, y, o: gp.fit_sites_(x, y, n_rounds=o['em_rounds'], m_steps=o['em_steps'], newton_iters=o['newton_iters'],
                                             start='prior')),
    'newton_softmax': (dict(create_clf=(lambda lik: lik == 'softmax', "q_init={q!r} fits the coupled sites of likelihood='softmax', "
                                        "got {lik!r}; the likelihoods with independent outputs have q_init='newton'")),
                       sites.check_softmax_supported,
                       lambda gp, x, y, o: gp.fit_q_softmax_(x, y, n_iters=o['newton_iters'], start='prior', n_f=o['site_samples'])),
    'em_softmax': (dict(create_clf=(lambda lik: lik == 'softmax', 'q_init={q!r} is variational EM on the coupled sites of '
                                    "likelihood='softmax', got {lik!r}; the likelihoods with independent outputs have q_init='em'")),
                   sites.check_softmax_differentiable,
                   lambda gp, x, y, o: gp.fit_softmax_sites_(x, y, n_rounds=o['em_rounds'], m_steps=o['em_steps'],
                                                             newton_iters=o['newton_iters'], start='prior', n_f=o['site_samples'])),
}
_Q_INITS = tuple(q for q, entry in _Q_INIT.items() if 'create_reg' in entry[0])      # create_reg (q_init=)
_CLF_Q_INITS = tuple(q for q, entry in _Q_INIT.items() if 'create_clf' in entry[0])        # create_clf (q_init=)


def _check_q_init(who, q_init, likelihood):
    """ValueError for a q_init the factory `who` does not accept, or one that does not apply to the likelihood's name."""
    accepted = _Q_INITS if who == 'create_reg' else _CLF_Q_INITS
    if q_init not in accepted:
        raise ValueError(f'{who}: q_init must be one of {sorted(accepted)}, got {q_init!r}')
    rule = _Q_INIT[q_init][0][who]
    if rule is not None and not rule[0](likelihood):
        raise ValueError(f'{who}: ' + rule[1].format(q=q_init, lik=likelihood))


def _fit_whole_dataset(gp, dataset, y, check, fit, who):
    """A factory's q_init: check the model, then on the current CUDA device load the whole data set (y: its targets as the fit
    takes them), run fit(gp, x, y) and bring the model home."""
    check(gp, who)
    home, dev = gp.z.device, torch.device('cuda', torch.cuda.current_device())
    x = dataset[torch.arange(len(dataset))][0].to(device=dev, dtype=torch.float32)
    y = y.to(dev)
    fit(gp.to(dev), x, y)
    gp.to(home)


def _check_init_names(who, z_init, lengthscale_init):
    if z_init not in _Z_INITS:
        raise ValueError(f'{who}: z_init must be one of {sorted(_Z_INITS)}, got {z_init!r}')
    if lengthscale_init not in _LENGTHSCALE_INITS:
        raise ValueError(f'{who}: lengthscale_init must be one of {sorted(_LENGTHSCALE_INITS)}, got {lengthscale_init!r}')


def _init_inducing(dataset, out_size, M, z_init, kmeans_iters):
    """z (out_size, M, D) of a new model.  'random': M random data points per output (vargp.py:207).  'kmeans' (not in the
    reference): Lloyd's algorithm from those very points over the task's data, on the current CUDA device (init.kmeans_inducing);
    the result comes back to the device and dtype the random route would have produced."""
    N = len(dataset)
    if z_init == 'random':
        return torch.stack([dataset[torch.randperm(N)[:M]][0] for _ in range(out_size)])
    x = dataset[torch.arange(N)][0]
    xd = x.to(device=torch.device('cuda', torch.cuda.current_device()), dtype=torch.float32)
    return init.kmeans_inducing(xd, out_size, M, n_iter=kmeans_iters).to(device=x.device, dtype=x.dtype)


def _greedy_candidates(dataset, out_size, M, n_candidates, who):
    """z_init='greedy', first half, at the point where the random route draws: the candidate rows of every output, one
    torch.randperm(N) each on the global generator (init.draw_candidates).  -> (x (N, D) as the dataset holds it, cand)."""
    N = len(dataset)
    cand = init.draw_candidates(N, out_size, n_candidates)
    if M > cand.shape[1]:
        raise ValueError(f"{who}: z_init='greedy' picks M = {M} inducing points from {cand.shape[1]} candidates "
                         f'(min(len(dataset), greedy_candidates))')
    return dataset[torch.arange(N)][0], cand


def _greedy_inducing(x, cand, M, kern, prior_log_mean, prev_params):
    """z_init='greedy', second half, once the kernel stands (not in the reference): greedy conditional-variance selection among
    the candidates on the current CUDA device (init.greedy_inducing).  Hyper vector: the kernel's own log_mean for a first task
    (after lengthscale_init, so 'median' and 'greedy' compose); for a later task the handed-over prior_log_mean -- the last
    task's trained hyper-posterior mean, the only informed value at that point -- and the selection starts from the previous
    tasks' inducing points.  The kernel code comes from the kernel's class whatever its route.  z returns on the dataset's
    device and dtype."""
    dev = torch.device('cuda', torch.cuda.current_device())
    theta = kern.log_mean.detach() if not prev_params or prior_log_mean is None else prior_log_mean
    nu2 = int(round(2 * kern.nu)) if isinstance(kern, MaternKernel) else 0
    z_prev = None
    if prev_params:
        z_prev = torch.cat([p['z'].detach().to(device=dev, dtype=torch.float32) for p in prev_params], dim=-2)
    xd = x.to(device=dev, dtype=torch.float32)
    z = init.greedy_inducing(xd, cand.shape[0], M, theta.to(dev), nu2=nu2, z_prev=z_prev, cand=cand)
    return z.to(device=x.device, dtype=x.dtype)


def _init_lengthscale(kern, dataset, lengthscale_init, first_task):
    """'median' (not in the reference): the first task's lengthscales start at the median pair distance of its data
    (init.median_lengthscale); a later task starts from the handed-over hyper-posterior whatever is asked."""
    if lengthscale_init == 'median' and first_task:
        kern.set_lengthscale_(init.median_lengthscale(dataset[torch.arange(len(dataset))][0]))
    return kern


class VARGP(nn.Module):
    def __init__(self, z_init, kernel, likelihood, n_var_samples=1, ep_var_mean=True, prev_params=None):
        super().__init__()
        self.var_mean_mask = float(ep_var_mean)
        self.fused_first_task = True     # VARGP.loss of a first-task model runs as one fused node (fused.py)
        self.fused_tasks = True          # ... and of a model with previous tasks as the block-structured program
        # native block programs: training programs per shape (+ spares while one is owned by a pending backward), ONE
        # forward-only program (moments only, no gradient buffers) sized for the widest batch seen, serving narrower ones
        self._tn_ops, self._tn_progs, self._tn_spares, self._tn_eval, self._tn_eval_exact = None, {}, {}, None, {}
        self._t0_progs, self._t0_spares = {}, {}       # first-task programs (csrc/elbo_t0.hip) of the autograd route, per shape
        # loss() on a native program returns lazy terms (lazy.py: no autograd graph for the caller's linear combination, the
        # backward is one program call); VARGP_LAZY_LOSS=0 or lazy_loss = False: three autograd tensors of one node, as before
        self.lazy_loss = os.environ.get('VARGP_LAZY_LOSS', '1') != '0'
        self._seed_cache, self._gbufs = {}, None
        # frozen earlier tasks: plain dicts, not buffers (same as the reference, vargp.py:17-20);
        # u_tril is materialised lazily on first use because that needs the device the params live on
        self.prev_params = [dict(z=p['z'], u_mean=p['u_mean'], u_tril_vec=p['u_tril_vec'])
                            for p in (prev_params or [])]
        self.M = z_init.size(-2)
        self.kernel = kernel
        self.n_v = n_var_samples
        self.likelihood = likelihood

        self.z = nn.Parameter(z_init.detach().clone())
        out_size = self.z.size(0)
        self.u_mean = nn.Parameter(torch.empty(out_size, self.M, 1).normal_(0., .5))
        # packed identity (vargp.py:32-33): diagonal entries 1 (softplus(1) = 1.3133 effective)
        eye_vec = torch.zeros(self.M * (self.M + 1) // 2)
        idx = torch.arange(self.M)
        eye_vec[idx * (idx + 1) // 2 + idx] = 1.0
        self.u_tril_vec = nn.Parameter(eye_vec.unsqueeze(0).repeat(out_size, 1))

    # ------------------------------------------------------------------------------------------
    def _prev(self, i):
        """previous task i as device tensors with its u_tril (vec2tril once, cached)."""
        p = self.prev_params[i]
        dev = self.z.device
        if 'u_tril' not in p or p['u_tril'].device != dev:
            for k in ('z', 'u_mean', 'u_tril_vec'):
                p[k] = p[k].detach().to(dev)
            with torch.no_grad():
                p['u_tril'] = vec2tril(p['u_tril_vec'])
        return p

    def compute_q(self, theta, cache=None):
        """Fold previous tasks into q(u_<t | theta) and q(u_<=t | theta)  (vargp.py:35-88).
        Returns mu_lt, S_lt, mu_leq_t, S_leq_t, z_leq_t."""
        # block form (gp_utils.block_joint) instead of the reference's chain of linear_joint calls: one
        # kernel matrix over the inducing points of all tasks, one factorisation; the joint over the earlier tasks is the
        # leading block of the joint over all of them
        prev = [self._prev(i) for i in range(len(self.prev_params))]
        n_lt = sum(p['z'].size(-2) for p in prev)
        z_leq_t = torch.cat([p['z'] for p in prev] + [self.z], dim=-2)
        L, T, mu_leq_t, S_leq_t = block_joint(self.kernel.compute(theta, z_leq_t), [p['u_mean'] for p in prev] + [self.u_mean],
                                              [p['u_tril'] for p in prev] + [vec2tril(self.u_tril_vec, self.M)])
        mu_lt = mu_leq_t[..., :n_lt, :].contiguous()
        S_lt = S_leq_t[..., :n_lt, :n_lt].contiguous()
        if isinstance(cache, dict):
            # factors of K(z_<t) + eps I and Lz_<t^-1 K(z_<t, z_t), as the chain's last step left them: leading blocks of L, T
            # and -- K_{t,<} = L_{t,<} L_<<^T -- the transposed off-diagonal block row of L
            cache['Lz_lt'] = L[..., :n_lt, :n_lt].contiguous()
            cache['Tz_lt'] = T[..., :n_lt, :n_lt].contiguous()
            cache['Lz_lt_Kz_lt_z_t'] = L[..., n_lt:, :n_lt].mT.contiguous()
        return mu_lt, S_lt, mu_leq_t, S_leq_t, z_leq_t

    def compute_pf_diag(self, theta, x, mu_leq_t, S_leq_t, z_leq_t, cache=None):
        """p(f) = int p(f | u_<=t) q(u_<=t): mean and variance diagonals (S, C, B)  (vargp.py:90-113)."""
        Kzz = self.kernel.compute(theta, z_leq_t)
        Kzx = self.kernel.compute(theta, z_leq_t, x)          # x (B, D) shared by all classes
        Kxx_diag = self.kernel.compute_diag(theta)
        return linear_marginal_diag(mu_leq_t, S_leq_t, Kzz, Kzx, Kxx_diag, cache=cache)

    # -- the block-structured native program (csrc/elbo_tn.hip) ------------------------------------------------------
    T0_TILE_UNITS_MAX = 16384      # csrc/elbo_t0.hip: kT0TileUnitsMax

    def first_task_as_block(self, B=None):
        """First-task models outside the range of the LDS-resident middles of csrc/elbo_t0.hip (M <= 104 and at most 16384
        (sample, class, 64-column) tile units, i.e. S C <= 2048 at B = 512) run as the one-block case of the block program
        (csrc/elbo_tn.hip: symmetric K_uu tiles, the factorisation's pivot chains beside the K_uf row slices, paired mid-size
        products).  Measured: Permuted-MNIST task 0 (M = 200, S = 10) 557 -> 572 steps/s.  (Until round 6 the limit was 2048
        units and the 64-sample Split-MNIST step took the block program: 314 steps/s against 372 on the multi-tile forms of the
        LDS-resident kernels.)  VARGP_T0_AS_TN=0 / 1 forces it; VARGP_T0_UNITS overrides the limit on both sides."""
        if self.prev_params:
            return False
        env = os.environ.get('VARGP_T0_AS_TN')
        if env is not None:
            return env == '1'
        n_v = 1 if self.kernel.map_est else self.n_v
        # B unknown (the trainer decides its program before it has seen a batch): the reference's 512.
        ntile = (int(B if B is not None else 512) + 63) // 64
        return self.M > 104 or n_v * self.z.size(0) * ntile > int(os.environ.get('VARGP_T0_UNITS', self.T0_TILE_UNITS_MAX))

    def _tn_applicable(self):
        return (self.fused_tasks and native_code(self.kernel) is not None and self.z.is_cuda
                and all(p['z'].shape[-2] == self.M for p in self.prev_params))

    def _use_block_program(self, B=None):
        """Does `loss` run on the block program (csrc/elbo_tn.hip)?  Models with previous tasks: ep_var_mean=True only (the
        KL of the ablation depends on a u_<t sample); first-task models: when first_task_as_block() says so -- the mask is
        irrelevant without previous tasks -- and fused_first_task has not been cleared."""
        if not self._tn_applicable():
            return False
        if self.prev_params:
            # ep_var_mean = False (the KL keeps the conditional prior's mean at n_v samples of u_<t): the same program with its
            # tn_nm_* kernels (csrc/elbo_tn.hip), for up to 16 samples
            n_v = 1 if self.kernel.map_est else self.n_v
            return self.var_mean_mask == 1.0 or (self.var_mean_mask == 0.0 and n_v <= 16)
        # (csrc/elbo_t0.hip is RBF-only: a native Matern first-task model is always the one-block case of the block program)
        return self.fused_first_task and (native_code(self.kernel) != 0 or self.first_task_as_block(B))

    def _tn_operands(self):
        """z_all (C, Mt, D), rk_all (C, nblk, M, NR): earlier tasks packed once, the last block is the program's scratch."""
        dev = self.z.device
        if self._tn_ops is None or self._tn_ops[0].device != dev:
            prev = [self._prev(i) for i in range(len(self.prev_params))]
            with torch.no_grad():
                self._tn_ops = fused.pack_tn_operands(prev, self.z.size(0), self.M, self.z.size(-1), dev)
        return self._tn_ops

    def _program(self, B, block):
        """The (cached) training program of this shape (block: csrc/elbo_tn.hip, otherwise csrc/elbo_t0.hip): descriptor +
        ~120 MB workspace are built once per shape, not per call.  While a loss() whose backward has not run yet owns its
        workspace (two losses combined before one backward), a spare of the same shape is used -- cached too, never
        re-allocated per step."""
        S = 1 if self.kernel.map_est else self.n_v
        shape = (S, self.z.size(0), self.M, self.z.size(-1), B, n_f(self.likelihood))
        cls, progs, spares, kw = fused.T0Program, self._t0_progs, self._t0_spares, {}
        if block:
            shape, cls, progs, spares = shape + (len(self.prev_params) + 1,), fused.TnProgram, self._tn_progs, self._tn_spares
            kw = dict(kernel_nu2=native_code(self.kernel))
        dev = self.z.device
        key = shape + tuple(kw.values())                 # (block programs: the kernel is part of the key, fused.TnProgram.key)
        prog = progs.get(key)
        if prog is None or prog.ws.device != dev:
            prog = progs[key] = cls(*shape, dev, self.kernel.map_est, **kw)
        elif prog.busy:
            pool = spares.setdefault(key, [])
            prog = next((q for q in pool if not q.busy and q.ws.device == dev), None)
            if prog is None:
                prog = cls(*shape, dev, self.kernel.map_est, **kw)
                pool.append(prog)
        return prog

    def _tn_program(self, B):
        return self._program(B, True)

    def _t0_program(self, B):
        return self._program(B, False)

    def _tn_eval_program(self, B, exact=False):
        """The forward-only program (predictive moments, no gradient buffers): one per model, carved for the widest batch
        asked for so far; narrower batches (the ragged last one of a sweep) run on it through the tile calls."""
        S = 1 if self.kernel.map_est else self.n_v
        key = (S, self.z.size(0), self.M, self.z.size(-1), n_f(self.likelihood), len(self.prev_params) + 1)
        kw = dict(map_est=self.kernel.map_est, forward_only=True, kernel_nu2=native_code(self.kernel))
        if exact:
            # D <= 32 (the direct distance form) has no tile mode: one small program per batch size, kept -- an accuracy sweep
            # with a ragged last batch would otherwise free and re-carve the single workspace twice per data set
            prog = self._tn_eval_exact.get(key + (B,))
            if prog is None or prog.ws.device != self.z.device:
                if len(self._tn_eval_exact) >= 8:
                    self._tn_eval_exact.clear()
                prog = self._tn_eval_exact[key + (B,)] = fused.TnProgram(*key[:4], B, *key[4:], self.z.device, **kw)
            return prog
        prog = self._tn_eval
        if (prog is None or prog.shape[4] < B or (prog.shape[:4] + prog.shape[5:]) != key
                or prog.ws.device != self.z.device):
            self._tn_eval = None          # release the old workspace before carving the wider one
            prog = self._tn_eval = fused.TnProgram(*key[:4], B, *key[4:], self.z.device, **kw)
        return prog

    def release_programs(self):
        """Drop every cached native program (workspaces of several GB at Mt ~ 2000); they are re-created on demand."""
        self._tn_progs, self._tn_spares, self._tn_eval, self._tn_eval_exact = {}, {}, None, {}
        self._t0_progs, self._t0_spares = {}, {}

    def _operands(self, detach=True):
        """What every native program reads of the model: (log_mean, log_logvar, prior_log_mean, prior_log_logvar, z, u_mean,
        u_tril_vec) -- detached for the program calls, the parameters themselves as inputs of the autograd node."""
        k = self.kernel
        ps = (k.log_mean, k.log_logvar, self.z, self.u_mean, self.u_tril_vec)
        log_mean, log_logvar, z, u_mean, u_tril_vec = [p.detach() for p in ps] if detach else ps
        return log_mean, log_logvar, k.prior_log_mean, k.prior_log_logvar, z, u_mean, u_tril_vec

    def forward(self, x, loss_cache=False):
        """x (B, D) -> pred_mu, pred_var (S, C, B); fills `loss_cache` with the KL ingredients if it is
        a dict  (vargp.py:115-175)."""
        if not torch.is_grad_enabled() and not isinstance(loss_cache, dict) and self._tn_applicable():
            # gradient-free evaluation (predict, accuracy sweeps): the native program, predictive moments only
            kern = self.kernel
            eps_theta = None if kern.map_est else noise.draw('eps_theta', (self.n_v, kern.log_mean.shape[0]), x.device)
            eps_theta = None if eps_theta is None else eps_theta.contiguous()
            # (D <= 32, the direct distance form, has no tile mode: exact-shape program)
            prog = self._tn_eval_program(x.size(0), exact=self.z.size(-1) <= 32)
            if prog.shape[4] == x.size(0):
                prog.forward(*self._operands(), *self._tn_operands(), x.contiguous(), None, eps_theta, None)
                mu, var = prog.moments()
            else:                                  # narrower than the program: x-independent part + one moments-only tile
                prog.sweep_begin(*self._operands(), *self._tn_operands(), eps_theta)
                mu, var = prog.sweep_moments(x.contiguous())
            return mu.clone(), var.clone()
        theta = self.kernel.sample_hypers(self.n_v)

        if self.prev_params:
            cache_q = dict()
            mu_lt, S_lt, mu_leq_t, S_leq_t, z_leq_t = self.compute_q(theta, cache=cache_q)
            pred_mu, pred_var = self.compute_pf_diag(theta, x, mu_leq_t, S_leq_t, z_leq_t)

            if isinstance(loss_cache, dict):
                Lz_Kzx = cache_q.pop('Lz_lt_Kz_lt_z_t').unsqueeze(0)          # (1, S, C, M<, M)
                Tz = cache_q.pop('Tz_lt').unsqueeze(0)
                Kzz = self.kernel.compute(theta, self.z).unsqueeze(0)
                # prior covariance Kzz - (Lz^-1 Kzx)^T (Lz^-1 Kzx): independent of u_<t
                prior_cov_t = ops.matmul(Lz_Kzx.mT, Lz_Kzx, D=Kzz, alpha=-1.0, beta=1.0)
                prior_L, prior_T = ops.chol_inv(prior_cov_t)
                if self.var_mean_mask == 1.0:
                    # var_mu - prior_mu = u_mean exactly; prior_mu itself is not needed
                    prior_mu_t = torch.zeros(1, 1, 1, 1, device=x.device)
                    var_mu_t = self.u_mean.squeeze(-1).unsqueeze(0).unsqueeze(0)
                else:
                    # u_<t ~ N(mu_<t, S_<t): Cholesky without jitter (MultivariateNormal, vargp.py:137-138)
                    Ls = ops.chol(S_lt, 0.0)
                    n_lt = mu_lt.shape[-2]
                    eps_u = noise.draw('eps_u', (self.n_v, theta.size(0), self.z.size(0), n_lt), x.device,
                                       sample_dim=1)
                    u_lt = mu_lt.unsqueeze(0) + ops.matmul(Ls.unsqueeze(0), eps_u.unsqueeze(-1), triA=LOWER)
                    Lz_u = ops.matmul(Tz, u_lt, triA=LOWER)
                    prior_mu_t = ops.matmul(Lz_Kzx.mT, Lz_u).squeeze(-1)       # (n_v, S, C, M)
                    var_mu_t = prior_mu_t * self.var_mean_mask + self.u_mean.squeeze(-1).unsqueeze(0).unsqueeze(0)
                var_L_cov_t = vec2tril(self.u_tril_vec, self.M).unsqueeze(0).unsqueeze(0)
                loss_cache.update(dict(var_mu_t=var_mu_t, var_L_cov_t=var_L_cov_t, prior_mu_t=prior_mu_t,
                                       prior_L_cov_t=prior_L, prior_T_cov_t=prior_T))
        else:
            cache_pf = dict()
            mu_leq_t = self.u_mean
            L_cov_leq_t = vec2tril(self.u_tril_vec, self.M)
            pred_mu, pred_var = self.compute_pf_diag(theta, x, mu_leq_t, rev_cholesky(L_cov_leq_t), self.z,
                                                     cache=cache_pf)
            if isinstance(loss_cache, dict):
                mu_t = mu_leq_t.squeeze(-1).unsqueeze(0).unsqueeze(0)            # q(u_1)
                L_cov_t = L_cov_leq_t.unsqueeze(0).unsqueeze(0)
                prior_mu_t = torch.zeros(1, 1, 1, 1, device=x.device)            # p(u_1) = N(0, Lz Lz^T)
                loss_cache.update(dict(var_mu_t=mu_t, var_L_cov_t=L_cov_t, prior_mu_t=prior_mu_t,
                                       prior_L_cov_t=cache_pf.pop('Lz').unsqueeze(0),
                                       prior_T_cov_t=cache_pf.pop('Tz').unsqueeze(0),
                                       # Lz^-1 (mu_q - 0) = Lz^-1 u_mean was already needed for the mean
                                       prior_d=cache_pf.pop('Lz_m').squeeze(-1).unsqueeze(0)))
        return pred_mu, pred_var

    def draw_t0_noise(self, x):
        """(eps_theta, eps_f) of one first-task step: the hyper-parameter noise of RBFKernel.sample_hypers
        (kernels.py:66-67; None under map_est) and the likelihood noise (likelihoods.py:26; None for an external
        likelihood -- Gaussian, Bernoulli -- which draws none)."""
        kern = self.kernel
        S = 1 if kern.map_est else self.n_v
        eps_theta = None if kern.map_est else noise.draw('eps_theta', (S, kern.log_mean.shape[0]), x.device)
        if is_external(self.likelihood):
            return eps_theta, None
        eps_f = noise.draw('eps_f', (S, self.likelihood.n_f, self.z.size(0), x.size(0)), x.device)
        return eps_theta, eps_f

    # -- lazy route (lazy.py) ---------------------------------------------------------------------------------------------------
    def _lazy_ok(self):
        """The five parameters are plain trainable leaves without hooks: the program's backward may write their .grad itself.
        Not for a model with an external likelihood (GaussianLikelihood and its sixth trainable tensor obs_log_var,
        BernoulliLikelihood): the likelihood runs between the program's forward and backward on the autograd-node route."""
        if not (self.lazy_loss and torch.is_grad_enabled()) or is_external(self.likelihood):
            return False
        k = self.kernel
        ps = (k.log_mean, self.z, self.u_mean, self.u_tril_vec) + (() if k.map_est else (k.log_logvar,))
        return all(p.requires_grad and p.is_leaf and not p._backward_hooks and p.is_cuda for p in ps)

    def _seed_tensor(self, coefs):
        t = self._seed_cache.get(coefs)
        if t is None or t.device != self.z.device:
            if len(self._seed_cache) >= 64:
                self._seed_cache.clear()
            t = self._seed_cache[coefs] = torch.tensor(coefs, dtype=torch.float32, device=self.z.device)
        return t

    def _grad_buffers(self):
        """([five buffers that become .grad], [five scratch buffers for accumulation into an existing .grad]), shapes of
        (log_mean, log_logvar, z, u_mean, u_tril_vec); each set is one allocation."""
        k = self.kernel
        ps = (k.log_mean, k.log_logvar, self.z, self.u_mean, self.u_tril_vec)
        if self._gbufs is None or self._gbufs[0][2].device != self.z.device or self._gbufs[0][2].shape != self.z.shape:
            self._gbufs = [fused._flat_views([p.shape for p in ps], self.z.device) for _ in range(2)]
        return self._gbufs

    def draw_u_noise(self, x):
        """eps_u (n_v, S, C, M<) of the u_<t ~ q(u_<t | theta) samples the ep_var_mean = False KL is averaged over (reference
        vargp.py:137-138); None for ep_var_mean = True models and first-task models."""
        if not self.prev_params or self.var_mean_mask == 1.0:
            return None
        S = 1 if self.kernel.map_est else self.n_v
        n_lt = sum(p['z'].shape[-2] for p in self.prev_params)
        return noise.draw('eps_u', (self.n_v, S, self.z.size(0), n_lt), x.device, sample_dim=1).contiguous()

    def loss(self, x, y):
        """(kl_hypers, kl_u, nll); the caller combines beta*kl_hypers + kl_u + (N/B)*nll
        (vargp.py:177-194, experiments/vargp.py:34)."""
        B = x.size(0)
        block = self._use_block_program(B)                      # csrc/elbo_tn.hip; otherwise, first task: csrc/elbo_t0.hip
        if block or (not self.prev_params and self.fused_first_task and native_code(self.kernel) == 0):
            lazy = self._lazy_ok()
            prog, packed = self._program(B, block), (self._tn_operands() if block else ())
            if lazy:
                return fused.elbo_lazy(self, x, y, prog, packed)
            # one autograd node.  External likelihoods (Gaussian, Bernoulli): the same programs with the likelihood left to the
            # caller (ext_lik), its value between forward and backward, its own parameter (obs_log_var) as a sixth input
            eps_theta, eps_f = self.draw_t0_noise(x)
            return fused.elbo_node(self._operands(detach=False), self.kernel.map_est, x, y, eps_theta, eps_f, prog, packed,
                                   eps_u=self.draw_u_noise(x),
                                   likelihood=self.likelihood if is_external(self.likelihood) else None)
        loss_cache = dict()
        pred_mu, pred_var = self(x, loss_cache=loss_cache)
        nll = self.likelihood.loss(pred_mu, pred_var, y)
        kl = gp_utils.mvn_kl(loss_cache.pop('var_mu_t'), loss_cache.pop('var_L_cov_t'),
                             loss_cache.pop('prior_mu_t'), loss_cache.pop('prior_L_cov_t'),
                             Tp=loss_cache.pop('prior_T_cov_t'), d=loss_cache.pop('prior_d', None))
        kl_u = kl.sum(dim=-1).mean(dim=0).mean(dim=0)
        kl_hypers = self.kernel.kl_hypers()
        return kl_hypers, kl_u, nll

    def elbo_tiled(self, x, y, tile, beta=1.0, scale=1.0, noise_seed=0):
        """ELBO terms and gradient over a whole data set x (N, D), y (N) swept in minibatch tiles of `tile` points
        (BASELINE config 5: N = 1e6, M = 2048): one hyper-sample set, the kernel matrix of the inducing points and its
        factorisation computed once, K_uf built tile by tile in HBM, every tile's share of the gradient accumulated on the
        device (fused.TnProgram.tiled_step).  Returns (kl_hypers, kl_u, nll summed over the data) and writes the gradient of
        beta kl_hypers + kl_u + scale nll into the .grad of the five trainable tensors.  ep_var_mean=True models only.
        Injected noise (noise.inject: eps_theta (S, D+1), eps_f (S, F, C, N)) is honoured; otherwise the program draws its
        own (counter-based generator keyed by `noise_seed`)."""
        assert self._tn_applicable() and (not self.prev_params or self.var_mean_mask == 1.0)
        if is_external(self.likelihood):
            raise NotImplementedError('elbo_tiled: the tiled sweep evaluates the softmax likelihood of integer labels; '
                                      f'{type(self.likelihood).__name__} models train through loss() or ElboTrainer')
        kern = self.kernel
        S = 1 if kern.map_est else self.n_v
        prog = self._tn_program(int(tile))       # honours a pending backward of VARGP.loss on the same shape
        eps_theta, eps_f = noise._injected.get('eps_theta'), noise._injected.get('eps_f')
        if eps_f is None:
            if prog._rng is None or prog._rng[0] != int(noise_seed):     # (re-)key the generator: a new seed is a new stream
                self._tiled_counter = torch.zeros(1, dtype=torch.int32, device=x.device)
                prog.set_rng(noise_seed, self._tiled_counter)
            eps_theta = None
        else:
            eps_theta = None if kern.map_est else eps_theta.to(x.device).contiguous()
            eps_f = eps_f.to(x.device)
        params = [kern.log_mean, kern.log_logvar, self.z, self.u_mean, self.u_tril_vec]
        grads = [torch.empty_like(p) for p in params]
        seeds = torch.tensor([beta, 1.0, scale], dtype=torch.float32, device=x.device)
        scal = prog.tiled_step(*self._operands(), *self._tn_operands(), x.contiguous(), y.contiguous(), seeds, grads, eps_theta, eps_f)
        for p, g in zip(params, grads):
            p.grad = g
        return scal[0].clone(), scal[1].clone(), scal[2].clone()

    def predict(self, x, tile=None):
        """Class probabilities (B, C)  (vargp.py:196-198; BernoulliLikelihood: per-output P(t = 1), not normalised over the
        outputs); for a GaussianLikelihood or StudentTLikelihood model the predictive means (S, C, B), for a PoissonLikelihood
        model the predicted rates (S, C, B).
        With `tile`, a large x is swept in blocks of `tile` points that share ONE hyper-sample and ONE set of x-independent
        factors (K_uu, its Cholesky / inverse, Lz^-1 m, Lz^-1 L_S): the same result as a single call on all of x, in bounded
        memory."""
        cat_dim = predict_batch_dim(self.likelihood)                 # blocks along B: last dim of (S, C, B), first of (B, C)
        if tile is None or x.size(0) <= tile:
            pred_mu, pred_var = self(x)
            return self.likelihood.predict(pred_mu, pred_var)
        out = []
        for _, mu, var in self._moment_sweep(x, tile):
            p = self.likelihood.predict(mu, var)
            out.append(p.clone() if p is mu else p)          # (the Gaussian mean may be a view the next tile overwrites)
        return torch.cat(out, dim=cat_dim)

    def _moment_sweep(self, x, tile):
        """The tiled sweep of predict / log_prob: yields (i, mu, var), the predictive moments (S, C, <= tile) of x[i:i + tile], for
        i = 0, tile, ...; every tile shares ONE hyper-sample and ONE set of x-independent factors.  The moments of a tile may be
        views that the next tile overwrites: consume (or clone) them before asking for the next."""
        if self.prev_params and not torch.is_grad_enabled() and self._tn_applicable() and self.z.size(-1) > 32:
            # the block program, forward only: K(z_<=t), its factorisation and the small products ONCE (vargp_elbo_tn_begin),
            # then K_uf, P, V2, W and the moments per tile.  (First-task models keep the per-op sweep below: with the factor of
            # S_u + eps I it needs two Mt^2 B products per tile where the block form needs three -- N = 1e6, M = 2048 sweep:
            # 0.93 s against 1.33 s.)
            kern = self.kernel
            eps_theta = None if kern.map_est else noise.draw('eps_theta', (self.n_v, kern.log_mean.shape[0]), x.device)
            prog = self._tn_eval_program(int(tile))
            prog.sweep_begin(*self._operands(), *self._tn_operands(), None if eps_theta is None else eps_theta.contiguous())
            for i in range(0, x.size(0), tile):
                mu, var = prog.sweep_moments(x[i:i + tile].contiguous())
                yield i, mu, var
            return
        theta = self.kernel.sample_hypers(self.n_v)
        if self.prev_params:
            _, _, mu_leq_t, S_leq_t, z_leq_t = self.compute_q(theta)
        else:
            mu_leq_t, z_leq_t = self.u_mean, self.z
            S_leq_t = rev_cholesky(vec2tril(self.u_tril_vec, self.M))
        prep = gp_utils.marginal_prepare(mu_leq_t, S_leq_t, self.kernel.compute(theta, z_leq_t))
        Kxx_diag = self.kernel.compute_diag(theta)
        for i in range(0, x.size(0), tile):
            mu, var, _ = gp_utils.marginal_apply(prep, self.kernel.compute(theta, z_leq_t, x[i:i + tile]), Kxx_diag)
            yield i, mu, var

    def log_prob(self, x, y, tile=None, per_output=False):
        """Held-out log predictive density of the targets y at x (N, D), per point: lpd (N,) = log of the mean over hyper-samples
        of the marginal likelihood of the point's whole target vector (likelihoods.py: log_prob; csrc/lpd.hip) -- log E_q[p(y)],
        not the ELBO's E_q[log p].  per_output=True: (lpd (N,), lpd_out (C, N)) with each output's own marginal (ValueError for
        the softmax, which has none).  y as loss() takes it: (N,) labels / shared targets, or (C, N) per-output targets.
        Evaluated under torch.no_grad() from the moment routes of predict: one self(x) call, or with `tile` and N > tile the
        same sweep as predict(tile=) (one hyper-sample draw and one factorisation for all tiles), targets sliced per tile."""
        with torch.no_grad():
            if tile is None or x.size(0) <= tile:
                return self.likelihood.log_prob(*self(x), y, per_output=per_output)
            out = [self.likelihood.log_prob(mu, var, y[..., i:i + tile], per_output=per_output)
                   for i, mu, var in self._moment_sweep(x, tile)]
            if per_output:
                return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out], dim=-1)
            return torch.cat(out)

    def uncertainty(self, x, tile=None, per_output=False):
        """Why the model is unsure about each point of x (N, D): likelihoods.Uncertainty(probs (N, C), total, aleatoric,
        epistemic (N,)), entropies in nats (likelihood.uncertainty; csrc/uncertainty.hip).  Over the model's samples (theta_s,
        f_sf) of the class distribution p(y | theta, f):
            total     = H[ E p(y | theta, f) ]      the entropy of the predictive distribution (of probs)
            aleatoric = E H[ p(y | theta, f) ]      noise: every sample agrees that the point is ambiguous (a class boundary)
            epistemic = max(total - aleatoric, 0)   the mutual information of the label and (theta, f): the samples disagree
                                                    with each other (an unseen class) -- the BALD score
        MulticlassSoftmax: 0 <= epistemic <= total <= log C; probs is predict's.  BernoulliLikelihood: per output on the 20-node
        rule, summed over the outputs (the one-vs-rest score, an upper bound on the joint quantity; total <= C log 2);
        per_output=True fills total_out, aleatoric_out, epistemic_out (C, N) too (ValueError for the softmax, which has no
        per-output parts).  For the probit link probs comes from the rule as well, not from predict's closed form
        Phi(mu / sqrt(1 + var)): the two differ by the rule's quadrature error (BernoulliLikelihood's docstring).  The
        regression likelihoods raise ValueError.
        Evaluated under torch.no_grad() from the moment routes of predict / log_prob: one self(x) call, or with `tile` and
        N > tile the same sweep (one hyper-sample draw and one factorisation for all tiles)."""
        with torch.no_grad():
            if tile is None or x.size(0) <= tile:
                return self.likelihood.uncertainty(*self(x), per_output=per_output)
            return cat_uncertainty([self.likelihood.uncertainty(mu, var, per_output=per_output)
                                    for _, mu, var in self._moment_sweep(x, tile)])

    def predict_f(self, x, full_cov=False):
        """The posterior over the latent functions at x (B, D), under torch.no_grad().  full_cov=False: what self(x) returns,
        (mu, var), both (S, C, B).  full_cov=True: (mu (S, C, B), cov (S, C, B, B)), the joint covariance of the B function
        values per hyper-sample and output: cov = K(x, x) - P^T P + W^T W with P = Lz^-1 Kzx, W = (Lz^-1 chol(S + eps I))^T P
        (csrc/pred_cov.hip), the convention of the variance route -- its diagonal is the pred_var of forward() for the same
        hyper-sample.  Every model (previous tasks or none, ep_var_mean on or off, any kernel, any likelihood) runs the
        composed route here: sample_hypers, compute_q, marginal_prepare, K(z, x), P, W, then the fused covariance op.
        Memory: cov takes 4 S C B^2 bytes (S C = 30, B = 4096: 2 GB).  A large x has to be handled in blocks by the caller;
        nothing here forms the cross-covariance between two blocks."""
        with torch.no_grad():
            if not full_cov:
                return self(x)
            theta = self.kernel.sample_hypers(self.n_v)
            if self.prev_params:
                _, _, mu_leq_t, S_leq_t, z_leq_t = self.compute_q(theta)
            else:
                mu_leq_t, z_leq_t = self.u_mean, self.z
                S_leq_t = rev_cholesky(vec2tril(self.u_tril_vec, self.M))
            prep = gp_utils.marginal_prepare(mu_leq_t, S_leq_t, self.kernel.compute(theta, z_leq_t))
            mu, P, W = gp_utils.marginal_apply_full(prep, self.kernel.compute(theta, z_leq_t, x))
            return mu, self.kernel.compute_cov(theta, x, P, W)

    def fit_q_(self, x, y, weights=None, temper=1.0):
        """Set q(u) of the current task to its closed-form optimum for the data x (N, D), y (N,) or (C, N) as loss() takes it
        (Titsias' collapsed bound; collapsed.fit_q_, not in the reference): u_mean and u_tril_vec are overwritten in place under
        torch.no_grad(), everything else is read at theta = kernel.log_mean.  One pass over the data on the device (ops.gram_moments:
        K(z, x) is never stored), first-task models and models with prev_params alike.  weights: None, (N,) or (C, N) per-point
        weights; temper: a factor on the likelihood.  -> collapsed.CollapsedFit(bound (C,) float64: the variational bound of this
        data at the optimum, per output; n_chunks).  GaussianLikelihood and ep_var_mean=True only (ValueError otherwise); RBFKernel,
        MaternKernel (any `native`) and DeepRBFKernel.
        The bound is the standard one, E_q log N(y | f, sigma^2) - KL(q(u_t) || p(u_t | u_<t)).  GaussianLikelihood.loss is the
        reference's -log N(y | mu, var + sigma^2) instead, so the fitted q(u) maximises this bound and is close to, but not exactly,
        the minimiser of kl_u + nll as VARGP.loss reports them; kl_u itself is the KL term of the bound."""
        return collapsed.fit_q_(self, x, y, weights=weights, temper=temper)

    def fit_q_newton_(self, x, y, n_iters=20, damping=1.0, tol=1e-6, weights=None, route=None, start='current'):
        """fit_q_'s counterpart for the Bernoulli, Poisson and Student-t likelihoods (sites.fit_q_newton_, not in the reference):
        full-batch natural-gradient (conjugate-computation) iterations on q(u) of this task at theta = kernel.log_mean, from the
        current u_mean / u_tril_vec (start='prior': from q(u) = the prior, the robust start for Poisson), which are overwritten in
        place under no_grad.  Each iteration replaces every likelihood term
        by a Gaussian site and refits q(u) in closed form (Newton's method on the bound for the log-concave likelihoods): two
        fused passes over x (N, D), K(z, x) never stored.  y as loss() takes it; weights None, (N,) or (C, N): per-point weights.
        -> sites.SiteFit(bound (n_iters + 1, C) float64 on the host, non-decreasing; n_iters; n_rejected; n_clamped; route).
        ValueError for MulticlassSoftmax (coupled outputs), GaussianLikelihood (use fit_q_), ep_var_mean=False and a damping
        outside (0, 1].  Student-t: see the caveat in sites.py (n_clamped)."""
        return sites.fit_q_newton_(self, x, y, n_iters=n_iters, damping=damping, tol=tol, weights=weights, route=route,
                                   start=start)

    def fit_q_softmax_(self, x, y, n_iters=20, damping=1.0, tol=1e-6, weights=None, route=None, start='current', n_f=32, seed=0):
        """fit_q_newton_'s counterpart for MulticlassSoftmax (sites.fit_q_softmax_, not in the reference): the same full-batch
        natural-gradient iterations on q(u) of this task, with one Gaussian site per (class, point) whose parameters come from
        ONE expectation over the softmax of all C marginals of the point -- a mean over n_f draws per point, their noise fixed by
        `seed` for the whole fit.  Three fused passes over x (N, D) per iteration, K(z, x) never stored.  y (N,) int64 class
        indices; weights None or (N,).  A candidate is accepted on the bound summed over the classes.
        -> sites.SiteFit(bound (n_iters + 1, 1) float64 on the host, non-decreasing; n_iters; n_rejected; n_clamped = 0; route).
        ValueError for any other likelihood, ep_var_mean=False, (C, N) weights and a bad damping, start or n_f.  Near the optimum
        the fit usually ends by a rejected step rather than by tol: see the caveat in sites.py."""
        return sites.fit_q_softmax_(self, x, y, n_iters=n_iters, damping=damping, tol=tol, weights=weights, route=route,
                                    start=start, n_f=n_f, seed=seed)

    def site_bound(self, x, y, weights=None, q=None, route=None):
        """The variational bound of x (N, D), y (as fit_q_newton_ takes it) per output for a Bernoulli, Poisson or Student-t model
        (sites.site_bound, not in the reference): (C,) float64 on the autograd graph of z, kernel.log_mean and the Student-t
        log_scale, with q(u_t) held FIXED in whitened coordinates -- q = (a_t, H_t) as sites.whitened_q returns it, None: the
        model's own q, where the value is fit_q_newton_(n_iters=0).bound[0].  One fused pass over the data forward and one
        backward (csrc/sites.hip: vargp_site_bound_bwd) plus one moment pass; K(z, x) is never stored.  The frozen tasks are
        constants; x, y and weights get no gradient.  ep_var_mean=True, exactly RBFKernel or MaternKernel (a DeepRBFKernel is
        refused: ValueError).  The hyper-prior is not part of the bound."""
        return sites.site_bound(self, x, y, weights=weights, q=q, route=route)

    def fit_sites_(self, x, y, n_rounds=5, m_steps=20, lr=1e-2, params=None, newton_iters=20, damping=1.0, tol=1e-6,
                   weights=None, route=None, start='current'):
        """Variational EM for the Bernoulli, Poisson and Student-t likelihoods (sites.fit_sites_): n_rounds of fit_q_newton_
        (E-step) and m_steps Yogi steps up sum_c site_bound over the chosen subset of {'z', 'kernel' (kernel.log_mean), 'lik'
        (the Student-t log_scale)} with q held fixed in whitened coordinates (M-step), then a last E-step.  An M-step that lowers
        the bound is undone and ends the fit.  The objective is the bound alone, WITHOUT the hyper-prior (kl_hypers): type-II
        maximum likelihood, not what VARGP.loss optimises.  -> sites.EMFit(bound (n_rounds + 1, C) float64 on the host, its
        sum over outputs non-decreasing; n_rounds; n_newton; stopped)."""
        return sites.fit_sites_(self, x, y, n_rounds=n_rounds, m_steps=m_steps, lr=lr, params=params, newton_iters=newton_iters,
                                damping=damping, tol=tol, weights=weights, route=route, start=start)

    def softmax_site_bound(self, x, y, weights=None, q=None, route=None, n_f=32, seed=0):
        """site_bound's counterpart for MulticlassSoftmax (sites.softmax_site_bound, not in the reference): fit_q_softmax_'s bound
        of x (N, D), y (N,) int64 -- the n_f-sample estimate with the noise of `seed`, summed over the classes -- as a (1,) float64
        on the autograd graph of z and kernel.log_mean, with q(u_t) held FIXED in whitened coordinates (q = (a_t, H_t) as
        sites.whitened_q returns it; None: the model's own q, where the value is fit_q_softmax_(n_iters=0, n_f, seed).bound[0]).
        The gradient is the exact derivative of the sampled value.  Two fused passes over the data forward and three backward
        (csrc/softmax_sites.hip: vargp_softmax_site_grads; csrc/sites.hip: vargp_site_transport_bwd; one moment pass); K(z, x) is
        never stored.  ep_var_mean=True, exactly RBFKernel or MaternKernel.  The hyper-prior is not part of the bound."""
        return sites.softmax_site_bound(self, x, y, weights=weights, q=q, route=route, n_f=n_f, seed=seed)

    def fit_softmax_sites_(self, x, y, n_rounds=5, m_steps=20, lr=1e-2, params=None, newton_iters=20, damping=1.0, tol=1e-6,
                           weights=None, route=None, start='current', n_f=32, seed=0):
        """Variational EM for MulticlassSoftmax (sites.fit_softmax_sites_): n_rounds of fit_q_softmax_ (E-step) and m_steps Yogi
        steps up softmax_site_bound over the chosen subset of {'z', 'kernel' (kernel.log_mean)} with q held fixed in whitened
        coordinates (M-step), all on the noise of (n_f, seed), then a last E-step.  An M-step that lowers the bound is undone and
        ends the fit.  The objective is the bound alone, WITHOUT the hyper-prior.  -> sites.EMFit(bound (n_rounds + 1, 1)
        float64 on the host, non-decreasing; n_rounds; n_newton; stopped)."""
        return sites.fit_softmax_sites_(self, x, y, n_rounds=n_rounds, m_steps=m_steps, lr=lr, params=params,
                                        newton_iters=newton_iters, damping=damping, tol=tol, weights=weights, route=route,
                                        start=start, n_f=n_f, seed=seed)

    def loo(self, x, y, weights=None, route=None, check=False, n_f=32, seed=0, tile=sites.COMPOSED_TILE):
        """Leave-one-out log predictive density of the current task's TRAINING data x (N, D), y (as this model's q(u) fit takes
        it) per point, without refits and without held-out data (loo.loo, not in the reference): q(v_t) is read as "prior x one
        Gaussian site per (output, point)", the site of each point is divided out in closed form (the EP / CVI cavity) and the
        likelihood's own log predictive density is taken at the cavity moments -- the units of log_prob.  ASSUMES that q(u_t) is
        a fixed point of the site iteration: exact LOO of the sparse model after fit_q_ (Gaussian), the standard approximation
        after fit_q_newton_ / fit_q_softmax_; after minibatch training the cavity of a point can be improper (r_n <= 0): such
        points come back NaN and are counted in n_unstable, and check=True adds `stationarity`, the relative distance of q's
        precision from "prior + sites" (small at a fixed point).  Evaluated at ONE hyper vector, theta = kernel.log_mean --
        unlike log_prob, which mixes over hyper-samples.  Every likelihood, first-task models and models with prev_params;
        ep_var_mean=True; RBF, Matern and deep-RBF kernels.  About the cost of one site pass over the data: one fused launch up
        to ops.SITE_MAX_MT inducing points over all tasks, composed from per-op kernels above it (route).  weights: those the fit
        used; n_f, seed: the draws of the softmax sites.
        -> loo.Loo(lpd (N,), lpd_out (C, N) or None for the softmax, mu, var (C, N): the cavity moments, n_unstable (C,),
        stationarity (C,) or None, route)."""
        return loo.loo(self, x, y, weights=weights, route=route, check=check, n_f=n_f, seed=seed, tile=tile)

    def collapsed_bound(self, x, y, weights=None, temper=1.0):
        """The bound fit_q_ returns -- the variational bound of x (N, D), y (N,) or (C, N) at the optimal q(u) of the current
        task -- as a (C,) float64 tensor on the autograd graph of z, kernel.log_mean and likelihood.obs_log_var
        (collapsed.collapsed_bound): maximise it to place inducing points and fit lengthscales and noise without any q(u)
        parameter (SGPR).  One fused pass over the data forward and one backward; K(z, x) is never stored.  q(u) is not touched;
        the frozen tasks are constants; x, y and weights get no gradient.  GaussianLikelihood, ep_var_mean=True, exactly
        RBFKernel or MaternKernel (a DeepRBFKernel is refused: ValueError).  The hyper-prior is not part of the bound."""
        return collapsed.collapsed_bound(self, x, y, weights=weights, temper=temper)

    def fit_collapsed_(self, x, y, n_steps=200, lr=1e-2, weights=None, temper=1.0, params=('z', 'kernel', 'noise')):
        """n_steps full-batch Yogi steps up sum_c collapsed_bound over the chosen subset of {'z', 'kernel' (kernel.log_mean),
        'noise' (obs_log_var)}, then fit_q_ once (collapsed.fit_collapsed_).  The objective is the bound alone, WITHOUT the
        hyper-prior (kl_hypers): type-II maximum likelihood, not what VARGP.loss optimises.  -> the bound per step, float64
        (n_steps + 1, C) on the host, the last row being fit_q_'s at the final parameters; one synchronisation, at the end."""
        return collapsed.fit_collapsed_(self, x, y, n_steps=n_steps, lr=lr, weights=weights, temper=temper, params=params)

    def sample_f(self, x, n_samples=1):
        """Joint draws of the latent functions at x (B, D): (n_samples, S, C, B), f = mu + chol(cov + JITTER I) eps with
        (mu, cov) = predict_f(x, full_cov=True) and eps = noise.draw('eps_fs', (n_samples, S, C, B)) (noise.inject can supply
        it); n_samples draws per hyper-sample.  The factorisation is ops.chol: a cov that is not positive definite after the
        jitter is reported by the Cholesky error mode in force (ops.set_cholesky_error_mode).  Memory: cov and its factor,
        2 x 4 S C B^2 bytes.  A large x must be sampled in blocks by the caller, each under the same injected eps_theta; the
        blocks are then independent given the hyper-sample (no cross-covariance between blocks is formed); sample_paths draws
        functions that can be evaluated at any number of points instead."""
        with torch.no_grad():
            mu, cov = self.predict_f(x, full_cov=True)
            S, C, B = mu.shape
            L = ops.chol(cov)
            eps = noise.draw('eps_fs', (int(n_samples), S, C, B), x.device)
            f = ops.bgemm(L, eps.permute(1, 2, 3, 0), D=mu.unsqueeze(-1), beta=1.0, triA=LOWER)       # (S, C, B, n)
            return f.permute(3, 0, 1, 2).contiguous()

    def sample_paths(self, n_paths=1, n_features=1024):
        """Pathwise draws of the latent functions (paths.PosteriorPaths): paths = gp.sample_paths(n); paths(x) -> (n, S, C, B),
        the layout of sample_f, for any x and as often as asked -- every call evaluates the SAME n functions per hyper-sample
        and output, at a cost linear in B (K(z, x) and n_features random Fourier features per point, csrc/rff.hip).  The
        draw is frozen: training the model afterwards does not change it.  Every model (previous tasks or none, ep_var_mean on
        or off, any kernel, any likelihood); the mean over draws is predict_f's, the covariance tends to predict_f's as
        n_features grows."""
        return PosteriorPaths(self, n_paths=n_paths, n_features=n_features)

    @staticmethod
    def create_clf(dataset, M=20, n_f=10, n_var_samples=3, prev_params=None,
                   ep_var_mean=True, map_est_hypers=False, dkl=False, kernel='rbf', native_kernel=False,
                   likelihood='softmax', link='probit', z_init='random', kmeans_iters=20, lengthscale_init='default',
                   greedy_candidates=4096, q_init='default', newton_iters=20, em_rounds=5, em_steps=20, site_samples=32):
        """Factory used by the experiment driver (vargp.py:200-243): inducing points at random data
        points per class, hyper-prior = previous task's hyper-posterior (popped from prev_params[-1],
        which is mutated like the reference does).  kernel: 'rbf' (the reference's), or 'matern12' / 'matern32' /
        'matern52' (MaternKernel; not with dkl).  native_kernel=True: the Matern model runs the native block program
        (MaternKernel(native=True)); an error with 'rbf' or dkl, which have no such choice.  likelihood: 'softmax' (the
        reference's MulticlassSoftmax(n_f)) or 'bernoulli' (BernoulliLikelihood(link), the integer labels read as one-vs-rest
        targets; n_f is then unused), with any kernel choice.  None of these is part of a checkpoint: give them again on reload.
        z_init: 'random' (the reference's) or 'kmeans' (k-means centres of the task's data from those random points, at most
        kmeans_iters Lloyd iterations on the current CUDA device) or 'greedy' (greedy conditional-variance selection among
        min(len(dataset), greedy_candidates) random data points per output under the model's own kernel, started from the
        previous tasks' inducing points when there are any: init.greedy_inducing; not with dkl).  lengthscale_init: 'default' (0.5, the reference's) or 'median'
        (the median pair distance of the task's data, first task only; not with dkl, whose features are untrained).
        q_init: 'default' (u_mean ~ N(0, 0.25), u_tril = the softplus identity, as the reference starts) or 'newton'
        (likelihood='bernoulli' only): once the inducing points and the lengthscale stand, fit_q_newton_(n_iters=newton_iters,
        start='prior')
        on the whole data set on the current CUDA device; the model returns on the device the default route returns it on.
        'em' (likelihood='bernoulli', RBF / Matern kernel): fit_sites_(n_rounds=em_rounds, m_steps=em_steps,
        newton_iters=newton_iters, start='prior') instead -- variational EM that also moves the inducing points and
        kernel.log_mean up the bound (without the hyper-prior).  'newton_softmax' (likelihood='softmax' only):
        fit_q_softmax_(n_iters=newton_iters, start='prior', n_f=site_samples) -- the same fit for the reference's own
        likelihood, with site_samples draws per point behind every expectation over the softmax.  'em_softmax'
        (likelihood='softmax' only, RBF / Matern kernel): fit_softmax_sites_(n_rounds=em_rounds, m_steps=em_steps,
        newton_iters=newton_iters, start='prior', n_f=site_samples) instead -- variational EM that also moves the inducing points
        and kernel.log_mean up the sampled bound (without the hyper-prior)."""
        _check_q_init('create_clf', q_init, likelihood)
        lik = make_clf_likelihood(likelihood, n_f, link)
        _check_init_names('create_clf', z_init, lengthscale_init)
        if dkl and lengthscale_init == 'median':
            raise ValueError("create_clf: lengthscale_init='median' measures distances between inputs; with dkl=True the kernel "
                             'acts on the features of an untrained network')
        if dkl and z_init == 'greedy':
            raise ValueError("create_clf: z_init='greedy' selects by the kernel between inputs; with dkl=True the kernel acts on "
                             'the features of an untrained network')
        if kernel not in _KERNEL_NU:
            raise ValueError(f'create_clf: kernel must be one of {sorted(_KERNEL_NU)}, got {kernel!r}')
        if dkl and kernel != 'rbf':
            raise ValueError('create_clf: dkl=True needs kernel="rbf" (DeepRBFKernel has no Matern head)')
        if native_kernel and (dkl or kernel == 'rbf'):
            raise ValueError('create_clf: native_kernel=True selects the native route of a Matern kernel (kernel="matern12" / '
                             '"matern32" / "matern52", dkl=False); the RBF kernel is always native, DeepRBFKernel never')
        out_size = torch.unique(dataset.targets).size(0)
        if z_init == 'greedy':
            x_all, cand = _greedy_candidates(dataset, out_size, M, greedy_candidates, 'create_clf')
            in_size = x_all.size(-1)
        else:
            z = _init_inducing(dataset, out_size, M, z_init, kmeans_iters)
            in_size = z.size(-1)

        first_task = not prev_params
        prior_log_mean, prior_log_logvar, phi_params = _hand_over_hyper_prior(prev_params, dkl)
        kern = _make_kernel(in_size, kernel, dkl, native_kernel, prior_log_mean, prior_log_logvar, map_est_hypers, phi_params)
        _init_lengthscale(kern, dataset, lengthscale_init, first_task)
        if z_init == 'greedy':
            z = _greedy_inducing(x_all, cand, M, kern, prior_log_mean, prev_params)
        gp = VARGP(z, kern, lik, n_var_samples=n_var_samples, ep_var_mean=ep_var_mean,
                   prev_params=prev_params)
        if q_init != 'default':
            o = dict(newton_iters=newton_iters, em_rounds=em_rounds, em_steps=em_steps, site_samples=site_samples)
            _fit_whole_dataset(gp, dataset, torch.as_tensor(dataset.targets).to(torch.int64), _Q_INIT[q_init][1],
                               lambda gp, x, y: _Q_INIT[q_init][2](gp, x, y, o), f'create_clf(q_init="{q_init}")')
        return gp

    @staticmethod
    def create_reg(dataset, M=20, n_var_samples=3, likelihood='gaussian', df=4.0, prev_params=None, ep_var_mean=True,
                   map_est_hypers=False, kernel='rbf', native_kernel=False, z_init='random', kmeans_iters=20,
                   lengthscale_init='default', greedy_candidates=4096, q_init='default', collapsed_steps=200, newton_iters=20,
                   em_rounds=5, em_steps=20):
        """Regression / count factory, the counterpart of create_clf (not in the reference): dataset[i] -> (x, y), dataset.targets
        (N,) (one output) or (N, C); inducing points at M random data points per output; hyper-prior = the previous task's
        hyper-posterior (popped from prev_params[-1], which is mutated as in create_clf).  likelihood: 'gaussian'
        (GaussianLikelihood), 'studentt' (StudentTLikelihood(df=df): robust to outliers) or 'poisson' (PoissonLikelihood:
        non-negative counts, log link; df is unused by the other two).  kernel / native_kernel / z_init / kmeans_iters /
        lengthscale_init / greedy_candidates: as create_clf, without dkl.
        q_init: 'default' (u_mean ~ N(0, 0.25), u_tril = the softplus identity, as the reference starts) or 'optimal' (Gaussian
        likelihood only): once the inducing points and the lengthscale stand, fit_q_ on the whole data set on the current CUDA
        device -- q(u) starts at its closed-form optimum and the trainer only has to move hyper-parameters and inducing points; the
        model returns on the device the default route returns it on.  'collapsed' (Gaussian likelihood, RBF / Matern kernel):
        fit_collapsed_(n_steps=collapsed_steps) instead -- inducing points, lengthscales and noise variance are first moved up
        the collapsed bound (without the hyper-prior), then q(u) is fitted.  'newton' (likelihood 'poisson' or 'studentt'; the
        Gaussian's own route is 'optimal'): fit_q_newton_(n_iters=newton_iters, start='prior') on the whole data set instead.
        'em' (likelihood 'poisson' or 'studentt', RBF / Matern kernel): fit_sites_(n_rounds=em_rounds, m_steps=em_steps,
        newton_iters=newton_iters, start='prior') -- variational EM that also moves inducing points, kernel.log_mean and the
        Student-t log_scale up the bound (without the hyper-prior); the prior start for the reason 'newton' uses it.
        None of likelihood, df, kernel and native_kernel is part of a checkpoint: give them again on reload.  A minibatch's
        targets go to loss() as (C, B) -- y.t() of a (B, C) batch -- or (B,)."""
        _check_q_init('create_reg', q_init, likelihood)
        if kernel not in _KERNEL_NU:
            raise ValueError(f'create_reg: kernel must be one of {sorted(_KERNEL_NU)}, got {kernel!r}')
        if native_kernel and kernel == 'rbf':
            raise ValueError('create_reg: native_kernel=True selects the native route of a Matern kernel (kernel="matern12" / '
                             '"matern32" / "matern52"); the RBF kernel is always native')
        _check_init_names('create_reg', z_init, lengthscale_init)
        targets = torch.as_tensor(dataset.targets)
        if targets.dim() not in (1, 2):
            raise ValueError(f'create_reg: dataset.targets must have shape (N,) or (N, C), got {tuple(targets.shape)}')
        out_size = 1 if targets.dim() == 1 else targets.size(1)
        lik = make_reg_likelihood(likelihood, out_size, df)
        if z_init == 'greedy':
            x_all, cand = _greedy_candidates(dataset, out_size, M, greedy_candidates, 'create_reg')
            in_size = x_all.size(-1)
        else:
            z = _init_inducing(dataset, out_size, M, z_init, kmeans_iters)
            in_size = z.size(-1)
        first_task = not prev_params
        prior_log_mean, prior_log_logvar, _ = _hand_over_hyper_prior(prev_params)
        kern = _make_kernel(in_size, kernel, False, native_kernel, prior_log_mean, prior_log_logvar, map_est_hypers, None)
        _init_lengthscale(kern, dataset, lengthscale_init, first_task)
        if z_init == 'greedy':
            z = _greedy_inducing(x_all, cand, M, kern, prior_log_mean, prev_params)
        gp = VARGP(z, kern, lik, n_var_samples=n_var_samples, ep_var_mean=ep_var_mean, prev_params=prev_params)
        if q_init != 'default':
            o = dict(collapsed_steps=collapsed_steps, newton_iters=newton_iters, em_rounds=em_rounds, em_steps=em_steps)
            _fit_whole_dataset(gp, dataset, (targets if targets.dim() == 1 else targets.t()).to(torch.float32), _Q_INIT[q_init][1],
                               lambda gp, x, y: _Q_INIT[q_init][2](gp, x, y, o), f'create_reg(q_init="{q_init}")')
        return gp
