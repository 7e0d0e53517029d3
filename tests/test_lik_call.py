"""CPU: the table-driven call path of the independent-output likelihoods (ops.lik_nll_fwd / lik_nll_bwd / lik_lpd and the public
one-liners on top of them).  The library is replaced by a recorder: for every kind, forward, backward and LPD must call the
expected symbol with exactly the arguments _lib._SIGNATURES declares -- pointers where it has pointers, host scalars where it
has scalars, each operand in its declared position.  No GPU: a wrong position never reaches a kernel here."""
import ctypes

import pytest
import torch

S, C, B = 2, 3, 5
WS_BYTES = {'bernoulli': 12, 'poisson': 24, 'studentt': 48}


class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.endswith('_workspace_bytes'):
            return lambda s, c, b: WS_BYTES[name.split('_')[1]]

        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def rec(monkeypatch):
    from vargp_amd import ops
    r = _Recorder()
    monkeypatch.setattr(ops, 'lib', lambda: r)
    monkeypatch.setattr(ops, 'require_device', lambda *t: None)
    monkeypatch.setattr(ops, 'stream_ptr', lambda: ctypes.c_void_p(0x57))
    monkeypatch.setattr(ops, 'scratch', lambda nbytes, device: torch.zeros((int(nbytes) + 3) // 4))
    return r


def _p(t):
    return None if t is None else t.data_ptr()


def _check(call, name, want):
    """`want`: the operands in ABI order -- a tensor or None stands for its pointer, 'ws' for the pointer of some live buffer, a
    tuple ('ws', pointer, nbytes) for the workspace pair, anything else for itself."""
    from vargp_amd import _lib
    got_name, got = call
    assert got_name == name
    flat = []
    for w in want:
        flat.extend(w[1:] if isinstance(w, tuple) else [w])
    types = _lib._SIGNATURES[name][1]
    assert len(got) == len(types) == len(flat), (name, len(got), len(types), len(flat))
    for i, (g, w, ty) in enumerate(zip(got, flat, types)):
        if ty is ctypes.c_void_p:
            assert isinstance(g, ctypes.c_void_p), (name, i, g)
            if isinstance(w, str):                       # 'ws': some live buffer
                assert g.value, (name, i)
            else:
                assert g.value == (w if isinstance(w, int) else _p(w)), (name, i)
        else:
            assert not isinstance(g, ctypes.c_void_p) and not torch.is_tensor(g), (name, i, g)
            assert type(g) is (float if ty is ctypes.c_float else int) and g == w, (name, i, g, w)


def _case(kind):
    """-> y, target tuple, extra, whether nll_bwd writes a parameter gradient"""
    from vargp_amd import ops
    if kind == 'bernoulli':
        y = torch.arange(B) % C
        return y, ops.bernoulli_target(y, C, B), (1,), False
    y = torch.rand(C, B)
    par = torch.zeros(C)
    extra = {'gauss': (par,), 'poisson': (), 'studentt': (par, 4.0, ops.studentt_lognorm(4.0))}[kind]
    return y, ops.reg_target(y, C, B), extra, kind != 'poisson'


KINDS = ['gauss', 'bernoulli', 'poisson', 'studentt']


@pytest.mark.parametrize('kind', KINDS)
def test_nll_plumbing_matches_the_declared_signature(rec, kind):
    from vargp_amd import ops
    mu, var = torch.zeros(S, C, B), torch.ones(S, C, B)
    _, target, extra, has_param = _case(kind)
    out, seed, gmu, gvar, gpar = torch.zeros(1), torch.ones(1), torch.zeros(S, C, B), torch.zeros(S, C, B), torch.zeros(C)
    has_ws = kind != 'gauss'
    ws = lambda live: [('ws', 'ws', WS_BYTES[kind]) if live else ('ws', None, 0)] if has_ws else []
    stream = [0x57]

    ops.lik_nll_fwd(kind, mu, var, target, extra, out)
    _check(rec.calls[-1], f'vargp_{kind}_nll_fwd', [mu, var, *target, *extra, out, S, C, B, *ws(True), *stream])

    grads = [seed, gmu, gvar] + ([gpar] if has_param else [])
    ops.lik_nll_bwd(kind, mu, var, target, extra, seed, gmu, gvar, gpar if has_param else None, nll=out)
    _check(rec.calls[-1], f'vargp_{kind}_nll_bwd', [mu, var, *target, *extra, *grads, out, S, C, B, *ws(True), *stream])
    # without the value: scratch only where a parameter gradient needs it
    ops.lik_nll_bwd(kind, mu, var, target, extra, seed, gmu, gvar, gpar if has_param else None)
    _check(rec.calls[-1], f'vargp_{kind}_nll_bwd', [mu, var, *target, *extra, *grads, None, S, C, B, *ws(has_param), *stream])
    assert len(rec.calls) == 3


@pytest.mark.parametrize('kind', KINDS)
def test_public_wrappers_call_the_expected_symbols(rec, kind):
    from vargp_amd import ops
    mu, var = torch.zeros(S, C, B, requires_grad=True), torch.ones(S, C, B, requires_grad=True)
    y, target, extra, has_param = _case(kind)
    par = extra[0].requires_grad_(True) if has_param else None
    nll = {'gauss': lambda: ops.gauss_nll(mu, var, y, par), 'bernoulli': lambda: ops.bernoulli_nll(mu, var, y, 'logit'),
           'poisson': lambda: ops.poisson_nll(mu, var, y), 'studentt': lambda: ops.studentt_nll(mu, var, y, par, 4.0)}[kind]()
    nll.backward()
    (f_name, f_args), (b_name, b_args) = rec.calls
    assert f_name == f'vargp_{kind}_nll_fwd' and b_name == f'vargp_{kind}_nll_bwd'
    tgt = [a if not torch.is_tensor(a) else 'ws' for a in target]              # (converted targets: some live pointer)
    host = list(extra[1 if has_param else 0:])
    ws = lambda live: ([('ws', 'ws', WS_BYTES[kind]) if live else ('ws', None, 0)] if kind != 'gauss' else [])
    _check(rec.calls[0], f_name, [mu, var, *tgt, *([par] if has_param else []), *host, 'ws', S, C, B, *ws(True), 0x57])
    _check(rec.calls[1], b_name, [mu, var, *tgt, *([par] if has_param else []), *host, 'ws', 'ws', 'ws',
                                  *(['ws'] if has_param else []), None, S, C, B, *ws(has_param), 0x57])
    assert mu.grad.shape == mu.shape and var.grad.shape == var.shape and (par is None or par.grad.shape == (C,))

    lpd = {'gauss': lambda po: ops.gauss_lpd(mu, var, y, par, per_output=po),
           'bernoulli': lambda po: ops.bernoulli_lpd(mu, var, y, 'logit', per_output=po),
           'poisson': lambda po: ops.poisson_lpd(mu, var, y, per_output=po),
           'studentt': lambda po: ops.studentt_lpd(mu, var, y, par, 4.0, per_output=po)}[kind]
    got = lpd(False)
    assert got.shape == (B,)
    _check(rec.calls[-1], f'vargp_{kind}_lpd', [mu, var, *tgt, *(['ws'] if has_param else []), *host, got, None, S, C, B, 0x57])
    got, out = lpd(True)
    assert out.shape == (C, B)
    _check(rec.calls[-1], f'vargp_{kind}_lpd', [mu, var, *tgt, *(['ws'] if has_param else []), *host, got, out, S, C, B, 0x57])


def test_gauss_target_is_reg_target():
    from vargp_amd import ops
    assert ops.gauss_target is ops.reg_target
    with pytest.raises(ValueError):
        ops.gauss_target(torch.zeros(B, C), C, B)
