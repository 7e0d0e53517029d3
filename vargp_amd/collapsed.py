"""The optimal q(u) of a Gaussian-likelihood model in closed form (Titsias' collapsed bound, SGPR) -- not in the reference, whose
q(u) is only ever moved by gradient steps.  `fit_q_` (VARGP.fit_q_, create_reg(q_init='optimal')) writes it into u_mean and
u_tril_vec and returns the bound's value at the optimum; for a Gaussian likelihood this is one natural-gradient step of length 1.

Everything happens at ONE hyper vector, theta = kernel.log_mean, in the whitened coordinates of gp_utils.block_joint: with
K' = K(z_<=t) + eps I = L L^T, T = L^-1 and v = T u, the posterior is q(v) = N(a, H H^T) with block-diagonal H, the blocks of the
frozen tasks i < t being a_i = T_ii m_i, H_i = T_ii Lu_i.  The data enter through two weighted moments of the cross-kernel,
Phi = sum_n w_n k_n k_n^T and c = sum_n w_n y_n k_n, k_n = k(z_<=t, x_n) (ops.gram_moments, csrc/moments.hip: K(z, X) is never
stored), and sw = sum_n w_n, syy = sum_n w_n y_n^2.  With A = T Phi T^T, tc = T c, beta = temper / sigma^2 per output, `<` the
earlier tasks and `t` the new block:

    b_t     = tc_t - A_{t,<} a_<
    Sigma_t = (I + beta A_tt)^-1           a_t = beta Sigma_t b_t
    u_mean  = L_tt a_t                     u_tril = chol(L_tt Sigma_t L_tt^T)
    bound   = -1/2 sw log(2 pi / beta)
              - 1/2 beta [syy - 2 a_<^T tc_< + a_<^T A_<< a_< + gamma^2 sw - tr A + sum_{i<t} tr(H_i^T A_ii H_i)]
              + 1/2 beta^2 b_t^T Sigma_t b_t - 1/2 logdet(I + beta A_tt)

`bound` = E_q log N(y | f, 1 / beta) - KL(q(v_t) || N(0, I)) at its maximum over (a_t, H_t): the standard variational bound of the
new task's data (tests/test_collapsed.py restates all of this in fp64, checks that the bound's gradient vanishes there and that the
closed form equals the evaluated bound).  Sigma_t has its eigenvalues in (0, 1] whatever the conditioning of K'.  u_tril comes
without a second factorisation: I + beta A_tt = U U^T with U UPPER triangular (the Cholesky factor of the matrix with rows and
columns reversed, reversed back), so Sigma_t = G G^T with G = U^-T lower triangular and u_tril = L_tt G.

CAVEAT: GaussianLikelihood.loss is the reference's -log N(y | mu, var + sigma^2) (its mean over outputs), not -E_q log p(y | f).
fit_q_ maximises the standard bound above, so the q(u) it writes is NOT exactly the minimiser of kl_u + nll as VARGP.loss
reports them (the two agree as the predictive variance becomes small against sigma^2); the loss is left as it is."""
import math
from collections import namedtuple

import torch

from . import ops
from .kernels import DeepRBFKernel, MaternKernel, RBFKernel
from .likelihoods import GaussianLikelihood
from .ops import LOWER, UPPER

CollapsedFit = namedtuple('CollapsedFit', 'bound n_chunks')
CollapsedFit.__doc__ = """bound (C,) float64: per output, the variational bound of the fitted data at the optimal q(u) (nats);
n_chunks: the number of chunks the moment kernel cut the N points into (ops.gram_moments_chunks)."""


def check_supported(gp, who='fit_q_'):
    """ValueError unless the closed form applies to the model: GaussianLikelihood, ep_var_mean=True, an RBF / Matern / deep-RBF
    kernel.  Needs no device."""
    if not isinstance(gp.likelihood, GaussianLikelihood):
        raise ValueError(f'{who}: the closed-form q(u) exists for GaussianLikelihood only (create_reg(likelihood="gaussian")), '
                         f'got {type(gp.likelihood).__name__}')
    if gp.var_mean_mask != 1.0:
        raise ValueError(f'{who}: supported for ep_var_mean=True models only (with ep_var_mean=False the mean of q(u_t) is not '
                         'u_mean alone)')
    if not isinstance(gp.kernel, RBFKernel):
        raise ValueError(f'{who}: supported kernels are RBFKernel, MaternKernel and DeepRBFKernel, got {type(gp.kernel).__name__}')


def _mv(A, v):
    """A v over the last dims, elementwise (fp64 on the device without a BLAS call): A (.., m, n), v (.., n) -> (.., m)."""
    return (A * v.unsqueeze(-2)).sum(-1)


def inv_softplus(d):
    """v with softplus(v) = d > 0 (the diagonal of vec2tril), in the dtype of d."""
    return torch.where(d > 20.0, d, torch.log(torch.expm1(d.clamp_max(20.0))))


def fit_q_(gp, x, y, weights=None, temper=1.0):
    """Set q(u_t) of the VARGP model `gp` to its optimum for the data x (N, D), y (N,) or (C, N) (as loss() takes it), in place and
    under no_grad; weights None, (N,) or (C, N), >= 0: per-point weights of the log-likelihood; temper: a factor on all of them
    (beta = temper / sigma^2).  First-task models and models with prev_params alike; hyper-parameters, inducing points and
    obs_log_var are read, not changed.  -> CollapsedFit(bound (C,) float64, n_chunks).  See the module docstring for the formulas
    and for how the bound relates to VARGP.loss."""
    check_supported(gp)
    kern = gp.kernel
    ops.require_device(gp.z, x, y, weights)
    with torch.no_grad():
        C, M, N = gp.z.size(0), gp.M, x.size(0)
        theta = kern.log_mean.detach().to(torch.float32).contiguous()
        prev = [gp._prev(i) for i in range(len(gp.prev_params))]
        z_all = torch.cat([p['z'] for p in prev] + [gp.z.detach()], dim=-2).contiguous()
        Mt = z_all.size(-2)
        n_lt = Mt - M
        yt, ldy = ops.reg_target(y, C, N)
        yt = yt.expand(C, N).contiguous() if ldy == 0 else yt
        wt = None
        if weights is not None:
            wt, ldw = ops.reg_target(weights, C, N)
            wt = wt.expand(C, N).contiguous() if ldw == 0 else wt
        deep = isinstance(kern, DeepRBFKernel)
        zf, xf = (kern.features(z_all), kern.features(x)) if deep else (z_all, x)
        nu2 = int(round(2 * kern.nu)) if isinstance(kern, MaternKernel) else 0

        # the only pass over the data
        Phi, c, sums = ops.gram_moments(theta, zf, xf, wt, yt, nu2)
        n_chunks = ops.gram_moments_chunks(C, Mt, N, zf.size(-1))

        L, T = ops.chol_inv(kern.compute(theta.unsqueeze(0), z_all)[0])                  # (C, Mt, Mt): as block_joint factorises
        A = ops.bgemm(ops.bgemm(T, Phi, triA=LOWER), T.mT, triB=UPPER).double()
        A = 0.5 * (A + A.mT)
        tc = ops.bgemm(T, c.unsqueeze(-1), triA=LOWER).squeeze(-1).double()
        sw, syy = sums[:, 0].double(), sums[:, 1].double()
        beta = float(temper) * (-gp.likelihood.obs_log_var.detach().double()).exp()      # (C,)
        g2 = (2.0 * theta[-1].double()).exp()

        # the frozen tasks: a_< and sum_i tr(H_i^T A_ii H_i)
        a_lt, trHAH, o = [], torch.zeros(C, dtype=torch.float64, device=x.device), 0
        for p in prev:
            n = p['z'].size(-2)
            T_ii = T[:, o:o + n, o:o + n].contiguous()
            a_lt.append(ops.bgemm(T_ii, p['u_mean'], triA=LOWER).squeeze(-1).double())
            H = ops.bgemm(T_ii, p['u_tril'], triA=LOWER, triB=LOWER).double().tril()
            A_ii = A[:, o:o + n, o:o + n]
            trHAH = trHAH + ((A_ii.unsqueeze(-1) * H.unsqueeze(-3)).sum(-2) * H).sum((-2, -1))
            o += n
        a_lt = torch.cat(a_lt, dim=-1) if a_lt else tc.new_zeros(C, 0)
        A_ll, A_tl, A_tt = A[:, :n_lt, :n_lt], A[:, n_lt:, :n_lt], A[:, n_lt:, n_lt:]
        b_t = tc[:, n_lt:] - _mv(A_tl, a_lt)

        # I + beta A_tt = U U^T, U upper: the Cholesky factor of the reversed matrix, reversed back; G = U^-T is lower
        Bm = torch.eye(M, dtype=torch.float64, device=x.device) + beta.view(C, 1, 1) * A_tt
        Lr, Tr = ops.chol_inv(Bm.flip(-2, -1).float().contiguous(), 0.0)
        G = Tr.mT.flip(-2, -1).contiguous()                                               # Sigma_t = G G^T
        G64 = G.double().tril()
        gb = _mv(G64.mT, b_t)
        quad = gb.square().sum(-1)                                                        # b_t^T Sigma_t b_t
        a_t = beta.unsqueeze(-1) * _mv(G64, gb)
        logdet = 2.0 * Lr.diagonal(dim1=-2, dim2=-1).double().log().sum(-1)

        L_tt = L[:, n_lt:, n_lt:].contiguous()
        u_mean = _mv(L_tt.double().tril(), a_t).unsqueeze(-1)
        u_tril = ops.bgemm(L_tt, G, triA=LOWER, triB=LOWER).tril()
        vec = ops.mat2trilvec(u_tril)
        idx = torch.arange(M, device=x.device)
        diag = idx * (idx + 1) // 2 + idx
        vec[:, diag] = inv_softplus(vec[:, diag].double()).float()

        fixed = syy - 2.0 * (a_lt * tc[:, :n_lt]).sum(-1) + (a_lt * _mv(A_ll, a_lt)).sum(-1) + g2 * sw \
            - A.diagonal(dim1=-2, dim2=-1).sum(-1) + trHAH
        bound = -0.5 * sw * (2.0 * math.pi / beta).log() - 0.5 * beta * fixed + 0.5 * beta.square() * quad - 0.5 * logdet

        gp.u_mean.copy_(u_mean.to(gp.u_mean.dtype))
        gp.u_tril_vec.copy_(vec.to(gp.u_tril_vec.dtype))
    return CollapsedFit(bound, n_chunks)
