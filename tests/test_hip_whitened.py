"""vargp_amd/whitened.py on the device, at C = 2, M = 20 plus one frozen task of 20 (Mt = 40), D = 2, N = 300: the premise that lets
ONE frame serve the fits (under no_grad) and the bounds (on the autograd graph) -- both give the same bits -- and that the fit and
the bound see the same alpha, Q."""
import pytest
import torch

from test_hip_site_bound import _model
from test_hip_sites import DEV

pytestmark = pytest.mark.gpu
C, M, D, N = 2, 20, 2, 300


@pytest.fixture(scope='module')
def fitted():
    """A probit model with one frozen task and a q(u_t) away from the default start.  -> (gp on DEV, x, y on DEV)"""
    gp0, x0, y0 = _model('probit', C, M, D, N, seed=22)
    gp0.fit_q_newton_(x0.to(DEV), y0.to(DEV), n_iters=3)
    prev = [dict(z=gp0.z.detach().clone(), u_mean=gp0.u_mean.detach().clone(), u_tril_vec=gp0.u_tril_vec.detach().clone())]
    gp, x, y = _model('probit', C, M, D, N, seed=23, prev=prev)
    x, y = x.to(DEV), y.to(DEV)
    gp.fit_q_newton_(x, y, n_iters=2)
    return gp, x, y


def test_frame_is_bitwise_the_same_with_and_without_grad(fitted):
    from vargp_amd import sites
    from vargp_amd.whitened import Frame, alpha_Q
    gp = fitted[0]
    q = sites.whitened_q(gp)
    with torch.no_grad():
        fr0 = Frame(gp)
        plain = (fr0.L, fr0.T, *alpha_Q(fr0, *q))
    fr1 = Frame(gp)
    graph = (fr1.L, fr1.T, *alpha_Q(fr1, *q))
    assert fr0.Mt == 2 * M and fr0.n_lt == M
    for name, p, g in zip(('L', 'T', 'alpha', 'Q'), plain, graph):
        assert g.requires_grad and not p.requires_grad, name
        assert torch.equal(p, g.detach()), name


def test_the_fit_and_the_frame_see_the_same_alpha_and_Q(fitted, monkeypatch):
    from vargp_amd import sites
    from vargp_amd.whitened import Frame, alpha_Q
    gp, x, y = fitted
    seen = []
    inner = sites._Problem._passes
    monkeypatch.setattr(sites._Problem, '_passes', lambda self, alpha, Q: seen.append((alpha.clone(), Q.clone())) or inner(self, alpha, Q))
    fit = gp.fit_q_newton_(x, y, n_iters=0)
    assert fit.n_iters == 0 and len(seen) == 1
    with torch.no_grad():
        alpha, Q = alpha_Q(Frame(gp), *sites.whitened_q(gp))
    assert torch.equal(seen[0][0], alpha) and torch.equal(seen[0][1], Q)
