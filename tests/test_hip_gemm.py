"""GPU: the batched GEMM (csrc/gemm.hip behind ops.bgemm / ops.matmul) on every tile shape, operand layout and strided
operand, element by element against fp64 on the host.

Tile shapes.  launch_gemm_epi chooses 128 x 128 x 16, 128 x 64 x 32 or 64 x 64 x 64 from the problem size, and the 128-wide
tiles only for problems far too large to restate on the host; vargp_tune_gemm_tile(1 / 2 / 3) forces each of them (0: the
library's own choice) on shapes small enough to check every element.

The bound is derived, not measured.  An entry of C = alpha A @ B + beta D is a sum of K products accumulated in fp32 by fused
multiply-adds (one rounding each), in whatever order the tile shape and the K slabs impose, scaled by alpha (one rounding)
and added to beta D (two more).  For any order of accumulation the error of the sum is at most gamma_K sum_k |a_ik b_kj| with
gamma_K = K u / (1 - K u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1); the three
roundings behind it and the second-order terms fit into four more u.  So, elementwise,

    |got - want|_ij <= (K + 4) 2^-24 (|alpha| (|A| @ |B|)_ij + |beta| |D|_ij) + 1e-30

(the absolute term only keeps 0 <= 0 true where both sides vanish).  Where a reduction over broadcast dimensions follows a
product (ops.matmul's backward), each of its n - 1 additions adds one more u.

Every product is written through `out=` into a window of a larger buffer filled with NaN -- rows further apart than N, and
matrices further apart than M rows -- and the buffer must be bit-identical outside the M x N windows afterwards: a store of
an edge tile that lands outside the result does not show in the values.  Operands that are placed with padding lie in
NaN-filled storage as well, so a padding element that reaches a result shows.

What the groups reach (plain-product instantiations; the distance epilogues have their own tile-by-tile test in
test_hip_matern.py):
  tiles x layouts x K    gemm_kernel<128,128,16>, <128,64,32>, <64,64,64>, each in four layouts, with scalar loads
                         (K % 4 != 0, or a transposed A with 150 rows) and with vector loads -- where tile 2 is the eight-wave
                         gemm_kernel_w8 in four layouts --, the pipelined fast path (A rows K-contiguous, K >= BK) with an
                         even and an odd number of full slabs, the guarded K tail, interior and edge epilogues with and
                         without D
  alignment              the switch from the vector to the scalar kernels (gemm_vec_ok) by base address, leading dimension
                         and batch stride alone
  small sizes            one-row / one-column / one-element results and sizes around one 128 x 64 tile on the 128-wide
                         tiles; the fast path of a transposed A (M % 4 == 0); K = 0
  triangular hints       K-range clipping, the long-tiles-first order, the zero-fill of a lower-triangular result above
                         the diagonal and the `col > row` masks, for BM == BN and BM != BN
  identity               a transposed or mirrored store of C
  grouped order          group_m = 8 with a ragged last group, with the XCD-compact map, on 64- and 128-row tiles
  matmul autograd        the backward products (transposed views, flipped hints, triC) and the reductions of broadcast
                         operands on the forced 128-wide tiles
"""
import itertools

import pytest
import torch

from oracle import vargp_oracle as orc

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24
TINY = 1e-30
NAN = float('nan')
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]


def _hn(shape, seed, scale=1.0):
    return (scale * orc.hash_normal(shape, seed)).float()


@pytest.fixture(scope='module')
def ops():
    from vargp_amd import ops as o
    return o


@pytest.fixture
def force_tile():
    """force_tile(t): every GEMM launch from here on uses tile shape t; always back to the library's choice afterwards"""
    from vargp_amd._lib import lib

    def force(t):
        assert lib().vargp_tune_gemm_tile(t) == 0
    try:
        yield force
    finally:
        lib().vargp_tune_gemm_tile(0)


_refs = {}


def _shared(key, make):
    """host-side inputs and fp64 references: computed once, shared by the cases that use them, never modified"""
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def _place(X, lead_pad=0, offset=0, batch_pad=0):
    """X on the device inside NaN-filled storage: rows `lead_pad` elements longer than X's, matrices `batch_pad` elements
    further apart than their size, the first element `offset` elements into the storage"""
    *bs, r, c = X.shape
    ld = c + lead_pad
    strides, s = [], r * ld + batch_pad
    for n in reversed(bs):
        strides.insert(0, s)
        s *= n
    flat = torch.full((offset + s,), NAN, device=DEV)
    v = torch.as_strided(flat, tuple(X.shape), (*strides, ld, 1), offset)
    v.copy_(X)
    return v


def _operand(X, trans, **kw):
    """the logical matrix X for bgemm, stored row-major (trans = 0) or transposed (a .mT view of row-major X^T)"""
    return _place(X.mT, **kw).mT if trans else _place(X, **kw)


def _into_window(bshape, M, N, product):
    """product(out) writes a (*bshape, M, N) result into a window of a larger NaN-filled buffer (rows N + 5 apart, M + 3 rows
    per matrix); -> the result on the host, after checking that nothing outside the windows has changed"""
    buf = torch.full((*bshape, M + 3, N + 5), NAN, device=DEV)
    ref_bits = buf.cpu().view(torch.int32)
    out = buf[..., 1:M + 1, 2:N + 2]
    ret = product(out)
    assert ret.data_ptr() == out.data_ptr()
    host = buf.cpu()
    got = host[..., 1:M + 1, 2:N + 2].clone()
    bits = host.view(torch.int32)
    bits[..., 1:M + 1, 2:N + 2] = ref_bits[..., 1:M + 1, 2:N + 2]
    assert torch.equal(bits, ref_bits), 'written outside the result'
    return got


def _ratio(got, want, mag, nround):
    """largest error in units of the bound nround 2^-24 mag + tiny (NaN if anything is NaN)"""
    return ((got.double() - want).abs() / (nround * U * mag + TINY)).max().item()


def _check(got, want, mag, nround, what):
    worst = _ratio(got, want, mag, nround)
    assert worst <= 1.0, f'{what}: error {worst:.3g} x the bound'     # (a NaN fails this too)


ALPHA, BETA = 0.5, 2.0


def _dense_case(M, N, K, seed=0):
    """A (2, 3, M, K), B (3, K, N): broadcast over the first batch dimension, D (2, 3, M, N) and the fp64 results with and
    without D, with their magnitudes"""
    def make():
        A, B, D = _hn((2, 3, M, K), 1 + seed), _hn((3, K, N), 2 + seed), _hn((2, 3, M, N), 3 + seed)
        AB = ALPHA * (A.double() @ B.double())
        mag = ALPHA * (A.double().abs() @ B.double().abs())
        return A, B, D, {False: (AB, mag), True: (AB + BETA * D.double(), mag + BETA * D.double().abs())}
    return _shared(('dense', M, N, K, seed), make)


def _dense_run(ops, case, M, N, K, tA, tB, with_d, what, kwA={}, kwB={}):
    A, B, D, refs = case
    Ad, Bd = _operand(A, tA, **kwA), _operand(B, tB, **kwB)
    Dd = D.to(DEV) if with_d else None
    got = _into_window((2, 3), M, N, lambda out: ops.bgemm(Ad, Bd, alpha=ALPHA, D=Dd, beta=BETA, out=out))
    want, mag = refs[with_d]
    _check(got, want, mag, K + 4, what)
    return got


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile', [0, 1, 2, 3])
def test_tiles_layouts_and_k_edges(ops, force_tile, tile):
    """150 x 200: interior and edge tiles of all three shapes.  K: the slab edges of BK = 16, 32 and 64; K % 4 != 0 gives
    scalar loads.  A transposed A of 150 rows has a leading dimension that is no multiple of 4 (scalar loads whatever K), so
    the transposed layouts run a second time with rows padded to 152, which the vector kernels take."""
    M, N = 150, 200
    force_tile(tile)
    for K in (1, 15, 16, 17, 31, 32, 33, 36, 64, 65, 100):
        case = _dense_case(M, N, K)
        for (tA, tB), with_d in itertools.product(LAYOUTS, (False, True)):
            for pad in ((0, 2) if tA else (0,)):
                _dense_run(ops, case, M, N, K, tA, tB, with_d, f'tile {tile} K {K} tA {tA} tB {tB} D {with_d} pad {pad}',
                           kwA=dict(lead_pad=pad))


@pytest.mark.parametrize('tile', [0, 1, 2, 3])
def test_alignment_switch(ops, force_tile, tile):
    """K = 36, every leading dimension a multiple of 4 (a transposed A padded to 152 rows): the vector kernels -- unless an
    operand starts one element into its storage, its leading dimension is padded by one, or its batch stride is no multiple
    of 4; each of these alone switches to the scalar kernels.  Same product: within the bound of fp64, and of the aligned
    result."""
    M, N, K = 150, 200, 36
    force_tile(tile)
    case = _dense_case(M, N, K)
    mag = case[3][True][1]
    for tA, tB in LAYOUTS:
        base = dict(lead_pad=2) if tA else {}
        aligned = _dense_run(ops, case, M, N, K, tA, tB, True, f'tile {tile} tA {tA} tB {tB} aligned', kwA=base)
        for name, kwA, kwB in [('A + 1', dict(base, offset=1), {}),
                               ('B + 1', base, dict(offset=1)),
                               ('A + 1, B + 1', dict(base, offset=1), dict(offset=1)),
                               ('lda + 1', dict(lead_pad=1), {}),
                               ('ldb + 1', base, dict(lead_pad=1)),
                               ('batch stride of A + 2', dict(base, batch_pad=2), {}),
                               ('batch stride of B + 2', base, dict(batch_pad=2))]:
            what = f'tile {tile} tA {tA} tB {tB} {name}'
            got = _dense_run(ops, case, M, N, K, tA, tB, True, what, kwA=kwA, kwB=kwB)
            _check(got, aligned.double(), mag, K + 4, what + ' against the aligned result')


@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('M,N', [(1, 1), (1, 200), (150, 1), (127, 65), (128, 64), (129, 63)])
def test_small_and_degenerate_sizes(ops, force_tile, tile, M, N):
    """K = 20: one full slab and a tail on the 128 x 128 x 16 tile, a tail only on 128 x 64 x 32."""
    force_tile(tile)
    case = _dense_case(M, N, 20, seed=10)
    for (tA, tB), with_d in itertools.product(LAYOUTS, (False, True)):
        _dense_run(ops, case, M, N, 20, tA, tB, with_d, f'tile {tile} {M} x {N} tA {tA} tB {tB} D {with_d}')


@pytest.mark.parametrize('M,N', [(1, 1), (150, 1), (129, 63)])
def test_k_zero(ops, M, N):
    """An empty sum: beta D, or zeros (what torch.matmul gives), exactly; nothing is launched, so there is no tile to force."""
    D = _hn((2, 3, M, N), 20)
    for tA, tB in LAYOUTS:
        A = torch.empty(2, 3, 0, M, device=DEV).mT if tA else torch.empty(2, 3, M, 0, device=DEV)
        B = torch.empty(3, N, 0, device=DEV).mT if tB else torch.empty(3, 0, N, device=DEV)
        got = _into_window((2, 3), M, N, lambda out: ops.bgemm(A, B, alpha=ALPHA, out=out))
        assert torch.equal(got, torch.zeros(2, 3, M, N))
        got = _into_window((2, 3), M, N, lambda out: ops.bgemm(A, B, alpha=ALPHA, D=D.to(DEV), beta=BETA, out=out))
        assert torch.equal(got, BETA * D)
        got = _into_window((2, 3), M, N, lambda out: ops.bgemm(A, B, D=D[0, :, :1].to(DEV), beta=BETA, out=out))
        assert torch.equal(got, (BETA * D[0, :, :1]).expand(2, 3, M, N))
    assert torch.equal(ops.bgemm(torch.empty(3, M, 0, device=DEV), torch.empty(0, N, device=DEV)).cpu(), torch.zeros(3, M, N))


# ---------------------------------------------------------------------------------------------
def _tri_case(n):
    def make():
        L1, L2, X = _hn((4, n, n), 5).tril(), _hn((4, n, n), 6).tril(), _hn((4, n, 77), 7)
        d = lambda t: t.double()                                                          # noqa: E731
        prods = {
            'LX': (d(L1) @ d(X), d(L1).abs() @ d(X).abs()),
            'LtX': (d(L1).mT @ d(X), d(L1).abs().mT @ d(X).abs()),
            'XtL': (d(X).mT @ d(L1), d(X).abs().mT @ d(L1).abs()),
            'XtLt': (d(X).mT @ d(L1).mT, d(X).abs().mT @ d(L1).abs().mT),
            'LL': ((d(L1) @ d(L2)).tril(), d(L1).abs() @ d(L2).abs()),
        }
        return L1, L2, X, prods
    return _shared(('tri', n), make)


@pytest.mark.parametrize('tile', [0, 1, 2, 3])
@pytest.mark.parametrize('n', [100, 200, 300])
def test_triangular_hints(ops, force_tile, tile, n):
    """The five products of test_hip_ops.py::test_bgemm_triangular_hints, and the two hints on the other storage order each
    (a lower A stored transposed, an upper A stored row-major; likewise B), on every tile shape.
    The ignored triangles hold ZEROS, not NaN: gemm_body clips the K range of a tile to the tile's edge (ke = min(ke, m0 + BM),
    ks = max(ks, m0), ...), not to the diagonal, so the ignored half of a diagonal tile IS loaded and multiplied.  What a hint
    promises is that a triangular matrix with zeros stored in its other half gives the full product."""
    force_tile(tile)
    L1, L2, X, prods = _tri_case(n)
    l1, l2, x = L1.to(DEV), L2.to(DEV), X.to(DEV)
    l1t, xt = l1.mT.contiguous(), x.mT.contiguous()       # L1^T (upper) and X^T stored row-major
    LOWER, UPPER = ops.LOWER, ops.UPPER
    for what, key, (M, N), product in [
        ('triA lower', 'LX', (n, 77), lambda out: ops.bgemm(l1, x, triA=LOWER, out=out)),
        ('triA upper, transposed view', 'LtX', (n, 77), lambda out: ops.bgemm(l1.mT, x, triA=UPPER, out=out)),
        ('triB lower', 'XtL', (77, n), lambda out: ops.bgemm(x.mT, l1, triB=LOWER, out=out)),
        ('triB upper, transposed view', 'XtLt', (77, n), lambda out: ops.bgemm(x.mT, l1.mT, triB=UPPER, out=out)),
        ('lower x lower -> lower', 'LL', (n, n), lambda out: ops.bgemm(l1, l2, triA=LOWER, triB=LOWER, triC=LOWER, out=out)),
        ('triA lower, transposed view', 'LX', (n, 77), lambda out: ops.bgemm(l1t.mT, x, triA=LOWER, out=out)),
        ('triA upper, row-major', 'LtX', (n, 77), lambda out: ops.bgemm(l1t, x, triA=UPPER, out=out)),
        ('triB upper, row-major', 'XtLt', (77, n), lambda out: ops.bgemm(xt, l1t, triB=UPPER, out=out)),
        ('triB lower, transposed view', 'XtL', (77, n), lambda out: ops.bgemm(xt, l1t.mT, triB=LOWER, out=out)),
        ('lower x lower -> lower, transposed views', 'LL', (n, n),
         lambda out: ops.bgemm(l1t.mT, l2.mT.contiguous().mT, triA=LOWER, triB=LOWER, triC=LOWER, out=out)),
    ]:
        got = _into_window((4,), M, N, product)
        want, mag = prods[key]
        _check(got, want, mag, n + 4, f'tile {tile} n {n} {what}')
        if key == 'LL':
            assert torch.equal(got.triu(1), torch.zeros_like(got)), f'tile {tile} n {n} {what}: strict upper triangle'


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tile', [0, 1, 2, 3])
def test_asymmetric_identity(ops, force_tile, tile):
    """I @ B and B^T @ I with an asymmetric B, in every layout: exact, and wrong if C is stored transposed or mirrored."""
    force_tile(tile)
    B = torch.arange(150 * 200, dtype=torch.float32).reshape(150, 200)
    eye = torch.eye(150)
    for tA, tB in LAYOUTS:
        got = _into_window((), 150, 200, lambda out: ops.bgemm(_operand(eye, tA), _operand(B, tB), out=out))
        assert torch.equal(got, B), f'tile {tile} tA {tA} tB {tB}: I @ B'
        got = _into_window((), 200, 150, lambda out: ops.bgemm(_operand(B.T, tA), _operand(eye, tB), out=out))
        assert torch.equal(got, B.T), f'tile {tile} tA {tA} tB {tB}: B^T @ I'


# ---------------------------------------------------------------------------------------------
def _grouped_case(M, N, K, nb):
    def make():
        # every block of 64 rows at a level of its own, so that a tile computed at another tile's place is far off
        level = (torch.arange(M) // 64 % 7 - 3.0).view(1, M, 1)
        A = (_hn((nb, M, K), 30) + level).float()
        B = _hn((K, N), 31)
        want = torch.einsum('bmk,kn->bmn', A.double(), B.double())
        mag = torch.einsum('bmk,kn->bmn', A.double().abs(), B.double().abs())
        return A, B, want, mag
    return _shared(('grouped', M, N, K, nb), make)


@pytest.mark.parametrize('tile,N,nb', [(0, 70, 120), (1, 70, 120), (2, 70, 120), (3, 70, 120), (1, 130, 76)])
def test_grouped_tile_order(ops, force_tile, tile, N, nb):
    """More than 4096 64 x 64 workgroups without a triangular hint: tiles are handed out eight tile rows at a time.  1100 rows
    are 18 tile rows of 64 (groups of 8, 8 and 2) or 9 of 128 (8 and 1): a ragged last group either way.  A skipped tile leaves
    NaN behind, a tile computed twice takes another one's place.  B row-major has a leading dimension of N (scalar loads),
    B transposed one of 8 (vector loads: the eight-wave kernel on tile 2).  With 70 columns the 128 x 128 tile has a single tile
    column, where the order within a group cannot go wrong; 130 columns give it two."""
    M, K = 1100, 8
    cdiv = lambda a, b: (a + b - 1) // b                                                  # noqa: E731
    assert cdiv(M, 64) * cdiv(N, 64) * nb > 4096, 'the shape has left the grouped order'
    assert cdiv(M, 64) % 8 != 0 and cdiv(M, 128) % 8 != 0, 'no ragged last group'
    force_tile(tile)
    A, B, want, mag = _grouped_case(M, N, K, nb)
    Ad = A.to(DEV)
    for tB in (0, 1):
        Bd = _operand(B, tB)
        got = _into_window((nb,), M, N, lambda out: ops.bgemm(Ad, Bd, out=out))
        _check(got, want, mag, K + 4, f'tile {tile} tB {tB}')


# ---------------------------------------------------------------------------------------------
def _autograd_case(n, dshape):
    def make():
        A, B, D, w = _hn((3, 4, n, n), 8).tril(), _hn((4, n, 9), 9), _hn(dshape, 10), _hn((3, 4, n, 9), 11)
        A64, B64, D64 = (t.double().requires_grad_(True) for t in (A, B, D))
        ref = -(A64 @ B64) + 0.5 * D64
        (ref * w.double()).sum().backward()
        aw, aA, aB = w.double().abs(), A.double().abs(), B.double().abs()
        mags = dict(out=aA @ aB + 0.5 * D.double().abs().expand(3, 4, n, 9),
                    A=aw @ aB.mT,                                                    # gA = alpha gC B^T, lower triangle
                    B=(aA.mT @ aw).sum(0),                                           # gB = sum_batch alpha A^T gC
                    D=0.5 * aw.sum(dim=[i for i in range(4) if dshape[i] == 1], keepdim=True))
        return A, B, D, w, ref.detach(), A64.grad.tril(), B64.grad, D64.grad, mags
    return _shared(('autograd', n, dshape), make)


@pytest.mark.parametrize('tile', [1, 2])
@pytest.mark.parametrize('dshape', [(1, 4, 150, 9), (1, 4, 1, 9)])
def test_matmul_autograd_on_the_128_wide_tiles(ops, force_tile, tile, dshape):
    """test_hip_ops.py::test_matmul_autograd_broadcast at n = 150, batch (3, 4), and with a D that is broadcast over rows as
    well: -(A @ B) + 0.5 D with a lower-triangular A, B shared by the first batch dimension.  Bounds as in the module
    docstring: gA is one product with K = 9; gB one with K = n and a sum over the three batch entries behind it (two more
    roundings); gD = 0.5 gC (one rounding) summed over the dimensions D is broadcast over (n_terms - 1 roundings)."""
    n = 150
    force_tile(tile)
    A0, B0, D0, w, ref, gA, gB, gD, mags = _autograd_case(n, dshape)
    A, B, D = (t.to(DEV).requires_grad_(True) for t in (A0, B0, D0))
    out = ops.matmul(A, B, D=D, alpha=-1.0, beta=0.5, triA=ops.LOWER)
    (out * w.to(DEV)).sum().backward()
    what = f'tile {tile} D {dshape}'
    _check(out.detach().cpu(), ref, mags['out'], n + 4, what + ' out')
    _check(A.grad.cpu(), gA, mags['A'], 9 + 4, what + ' gA')
    _check(B.grad.cpu(), gB, mags['B'], n + 4 + 2, what + ' gB')
    _check(D.grad.cpu(), gD, mags['D'], 1 + w.numel() // D0.numel() - 1, what + ' gD')
