"""The whitened posterior of a VARGP model at ONE hyper vector -- what collapsed.py (the closed-form q(u) of a Gaussian likelihood)
and sites.py (the natural-gradient site fits and the site bound) are both built on -- and the model checks the two share.

The coordinates are those of gp_utils.block_joint: theta = kernel.log_mean, z_<=t the inducing points of all tasks (the frozen ones
first), K' = K(z_<=t) + eps I = L L^T, T = L^-1 and v = T u.  The posterior is q(v) = N(a, H H^T) with a = (a_<, a_t) and
block-diagonal H, the blocks of the frozen tasks i < t being a_i = T_ii m_i, H_i = T_ii Lu_i (`<` the earlier tasks, `t` the new
block).  With k_n = k(z_<=t, x_n):

    alpha = T^T a,   Q = T^T (I - H H^T) T            (so that q(f_n) = N(alpha . k_n, gamma^2 - k_n^T Q k_n))      alpha_Q
    A = T Phi T^T,   tc = T c                         for data moments Phi = sum_n w_n k_n k_n^T, c = sum_n v_n k_n  whiten_moments
    KL(q(v_t) || N(0, I)) = 1/2 (|a_t|^2 + |H_t|_F^2 - M - 2 sum log diag H_t)                                       kl_standard
    u_mean = L_tt a_t,   u_tril = L_tt H_t            and back: a_t = T_tt u_mean, H_t = T_tt L_u                    write_q_, read_q

A symmetric positive B (I + beta A_tt, or the precision P of q(v_t)) is inverted WITHOUT a second factorisation of its inverse:
B = U U^T with U UPPER triangular (the Cholesky factor of the matrix with rows and columns reversed, reversed back), so
B^-1 = G G^T with G = U^-T lower triangular, and u_tril = L_tt G (reversed_chol).

Every piece is written on differentiable ops (ops.chol_inv, ops.matmul) or in fp64 elementwise torch, so under no_grad it is the
plain computation (the fits) and otherwise it sits on the autograd graph of gp.z and kernel.log_mean (the bounds); the frozen
tasks' inducing points and q(u) are constants, their whitened moments depend on theta through T and are differentiated.  The
forward of ops.matmul is ops.bgemm with the same descriptor, so the two uses agree bitwise (tests/test_hip_whitened.py).  Only
read_q and write_q_ are not: the model's q(u_t) is read detached and written under no_grad.

ORDER.  Autograd runs a graph's nodes in the reverse of the order of their creation and adds the gradients of a tensor with several
consumers in that order; fp32 addition does not associate.  Frame therefore computes nothing before it is asked (the factors, the
diagonal blocks, the frozen tasks' moments: on first use), so that a caller decides where they stand among its own nodes:
collapsed._whitened_bound makes its pass over the data BEFORE the factorisation, and theta has three consumers there.

Not here: gp_utils.block_joint and the minibatch ELBO path use the same algebra on a sample-batched layout (S hyper samples, the
native block program); see DESIGN.md, "What collapsed.py and sites.py share"."""
from functools import cached_property

import torch

from . import ops
from .kernels import DeepRBFKernel, MaternKernel, RBFKernel
from .ops import LOWER, UPPER


def mv(A, v):
    """A v over the last dims, elementwise (fp64 on the device without a BLAS call): A (.., m, n), v (.., n) -> (.., m)."""
    return (A * v.unsqueeze(-2)).sum(-1)


def inv_softplus(d):
    """v with softplus(v) = d > 0 (the diagonal of vec2tril), in the dtype of d."""
    return torch.where(d > 20.0, d, torch.log(torch.expm1(d.clamp_max(20.0))))


def check_model(gp, who, check_likelihood, deep=None):
    """ValueError unless `check_likelihood(gp.likelihood, who)` passes, the model has ep_var_mean=True and an RBF / Matern /
    deep-RBF kernel.  deep: None, or the text with which a DeepRBFKernel is refused FIRST by a differentiable bound, whose kernel
    must then be exactly RBFKernel or MaternKernel.  Needs no device."""
    if deep is not None and isinstance(gp.kernel, DeepRBFKernel):
        raise ValueError(f'{who}: DeepRBFKernel is not supported ({deep}')
    check_likelihood(gp.likelihood, who)
    if gp.var_mean_mask != 1.0:
        raise ValueError(f'{who}: supported for ep_var_mean=True models only (with ep_var_mean=False the mean of q(u_t) is not '
                         'u_mean alone)')
    if not isinstance(gp.kernel, RBFKernel):
        raise ValueError(f'{who}: supported kernels are RBFKernel, MaternKernel and DeepRBFKernel, got {type(gp.kernel).__name__}')
    if deep is not None and type(gp.kernel) not in (RBFKernel, MaternKernel):
        raise ValueError(f'{who}: supported kernels are exactly RBFKernel and MaternKernel, got {type(gp.kernel).__name__}')


class Frame:
    """The whitened frame of the model `gp` at its current parameters: theta (D+1,) fp32, z_all (C, Mt, D) the inducing points of
    all tasks, C, M, Mt, n_lt = Mt - M, nu2 (0 = RBF, 1 | 3 | 5 = Matern) at once; L, T (C, Mt, Mt), the new block's L_tt, T_tt
    and the frozen tasks' moments on first use (the module docstring says why)."""

    def __init__(self, gp):
        self.kern = kern = gp.kernel
        self.C, self.M = gp.z.size(0), gp.M
        self.theta = kern.log_mean.to(torch.float32).contiguous()
        self.prev = [gp._prev(i) for i in range(len(gp.prev_params))]
        self.z_all = torch.cat([p['z'] for p in self.prev] + [gp.z], dim=-2).contiguous()
        self.Mt = self.z_all.size(-2)
        self.n_lt = self.Mt - self.M
        self.nu2 = int(round(2 * kern.nu)) if isinstance(kern, MaternKernel) else 0

    def operands(self, x):
        """(zf, xf): the inducing points and the inputs x (N, D) as the data passes take them (a DeepRBFKernel's features)."""
        k = self.kern
        return (k.features(self.z_all), k.features(x)) if isinstance(k, DeepRBFKernel) else (self.z_all, x)

    # (L, T) (C, Mt, Mt): as block_joint factorises
    factors = cached_property(lambda self: ops.chol_inv(self.kern.compute(self.theta.unsqueeze(0), self.z_all)[0]))
    L = property(lambda self: self.factors[0])
    T = property(lambda self: self.factors[1])
    L_tt = cached_property(lambda self: self.L[:, self.n_lt:, self.n_lt:].contiguous())
    T_tt = cached_property(lambda self: self.T[:, self.n_lt:, self.n_lt:].contiguous())
    eye = cached_property(lambda self: torch.eye(self.Mt, dtype=torch.float32, device=self.z_all.device))

    @cached_property
    def frozen(self):
        """The frozen tasks' whitened moments: (a_< (C, n_lt) float64, [H_i (C, M_i, M_i) fp32, lower] in the order of the tasks)."""
        T, a_lt, H_lt, o = self.T, [], [], 0
        for p in self.prev:
            n = p['z'].size(-2)
            T_ii = T[:, o:o + n, o:o + n].contiguous()
            a_lt.append(ops.matmul(T_ii, p['u_mean'], triA=LOWER).squeeze(-1).double())
            H_lt.append(ops.matmul(T_ii, p['u_tril'], triA=LOWER, triB=LOWER).tril())
            o += n
        return torch.cat(a_lt, dim=-1) if a_lt else torch.zeros(self.C, 0, dtype=torch.float64, device=T.device), H_lt

    @cached_property
    def Hb(self):
        """The block-diagonal H (C, Mt, Mt) fp32 with the frozen tasks' blocks filled in; alpha_Q writes the new task's block
        INTO it, so on the autograd graph a frame serves one q."""
        Hb, o = torch.zeros(self.C, self.Mt, self.Mt, dtype=torch.float32, device=self.T.device), 0
        for H in self.frozen[1]:
            n = H.size(-1)
            Hb[:, o:o + n, o:o + n] = H
            o += n
        return Hb


def alpha_Q(fr, a_t, H_t):
    """q(v_t) = N(a_t, H_t H_t^T), a_t (C, M) float64, H_t (C, M, M) fp32 lower, joined with the frozen tasks of the frame:
    -> (alpha (C, Mt), Q (C, Mt, Mt) symmetrised), fp32 contiguous."""
    Hb = fr.Hb
    alpha = mv(fr.T.mT.double(), torch.cat([fr.frozen[0], a_t], dim=-1)).float().contiguous()
    Hb[:, fr.n_lt:, fr.n_lt:] = H_t
    Q = ops.matmul(ops.matmul(fr.T.mT, fr.eye - ops.matmul(Hb, Hb.mT)), fr.T)
    return alpha, (0.5 * (Q + Q.mT)).contiguous()


def whiten_moments(T, Phi, c):
    """-> (A = T Phi T^T (C, Mt, Mt), symmetrised in fp64; tc = T c (C, Mt)), float64."""
    A = ops.matmul(ops.matmul(T, Phi, triA=LOWER), T.mT, triB=UPPER).double()
    return 0.5 * (A + A.mT), ops.matmul(T, c.unsqueeze(-1), triA=LOWER).squeeze(-1).double()


def reversed_chol(B):
    """B (C, M, M) float64, symmetric positive = U U^T with U upper triangular -> (Lr, G) fp32: Lr the Cholesky factor of B with
    rows and columns reversed (logdet B = 2 sum log diag Lr) and G = U^-T with B^-1 = G G^T, lower triangular in exact
    arithmetic and NOT cleared above the diagonal."""
    Lr, Tr = ops.chol_inv(B.flip(-2, -1).float().contiguous(), 0.0)
    return Lr, Tr.mT.flip(-2, -1).contiguous()


def kl_standard(a_t, H_t):
    """KL(N(a_t, H_t H_t^T) || N(0, I)) (C,) float64: a_t (C, M) float64, H_t (C, M, M) lower triangular, read in fp64."""
    H64 = H_t.double()
    return 0.5 * (a_t.square().sum(-1) + H64.square().sum((-2, -1)) - a_t.size(-1)
                  - 2.0 * H64.diagonal(dim1=-2, dim2=-1).log().sum(-1))


def read_q(gp, T_tt):
    """The model's q(u_t) in whitened coordinates: -> (a_t = T_tt u_mean (C, M) float64, H_t = T_tt L_u (C, M, M) fp32 lower,
    L_u (C, M, M)), detached."""
    L_u = ops.vec2tril(gp.u_tril_vec.detach().float(), gp.M)
    a_t = ops.matmul(T_tt, gp.u_mean.detach().float(), triA=LOWER).squeeze(-1).double()
    return a_t, ops.bgemm(T_tt, L_u, triA=LOWER, triB=LOWER).tril(), L_u


def write_q_(gp, L_tt, a_t, H_t):
    """u_mean = L_tt a_t and u_tril = L_tt H_t into gp.u_mean / gp.u_tril_vec (the diagonal through the inverse softplus of
    vec2tril).  Under no_grad."""
    u_mean = mv(L_tt.double().tril(), a_t).unsqueeze(-1)
    u_tril = ops.bgemm(L_tt, H_t, triA=LOWER, triB=LOWER).tril()
    vec = ops.mat2trilvec(u_tril)
    idx = torch.arange(gp.M, device=vec.device)
    diag = idx * (idx + 1) // 2 + idx
    vec[:, diag] = inv_softplus(vec[:, diag].double()).float()
    gp.u_mean.copy_(u_mean.to(gp.u_mean.dtype))
    gp.u_tril_vec.copy_(vec.to(gp.u_tril_vec.dtype))


def rows(t, C, N):
    """Targets or weights (N,) or (C, N) as fp32 (C, N) rows, detached: a shared row is written out for every output."""
    t, ld = ops.reg_target(t, C, N)
    return t.expand(C, N).contiguous() if ld == 0 else t
