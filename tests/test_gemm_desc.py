"""CPU: the operand descriptor of the batched GEMM (ops._gemm_desc) addresses exactly the right elements.

A small interpreter walks a GemmDesc the way gemm.hip does -- per batch index `base + i0 s[0] + i1 s[1] + i2 s[2]`, per element
`row * ld + col` (`col * ld + row` for a transposed operand), offsets in fp32 elements from the descriptor's pointers -- over
flat views of the tensors' storages.  Every offset it forms has to lie inside the storage of the tensor it belongs to (so a
wrong leading dimension or stride is caught here, without an out-of-bounds access on a device), no result element may be
written twice, nothing outside the result window may be written, and the result has to equal alpha A @ B + beta D.  Operands
are small integers and alpha = 0.5, beta = 2, so fp64 arithmetic is exact on both sides and the comparison is `==`."""
import itertools

import pytest
import torch

from vargp_amd import ops

ALPHA, BETA = 0.5, 2.0


def _ints(shape, seed, offset=0):
    """integer-valued fp32 tensor; `offset`: it starts that many elements into its storage"""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    flat = torch.randint(-9, 10, (n + offset,), generator=g).float()
    return flat[offset:].view(*shape)


def _flat(t, address):
    """(all of t's storage as a list, index of `address` in it)"""
    st = t.untyped_storage()
    byte = address - st.data_ptr()
    assert byte % 4 == 0 and 0 <= byte <= st.nbytes(), 'descriptor pointer outside its tensor'
    return torch.empty(0, dtype=torch.float32).set_(st).tolist(), byte // 4


def interpret(d, keep, C):
    """C's storage (fp64, NaN where nothing was written) after the product `d` describes, computed the way the kernel
    addresses memory."""
    fa, oa = _flat(keep[0], d.A)
    fb, ob = _flat(keep[1], d.B)
    fd, od = _flat(keep[2], d.D) if d.D else (None, 0)
    nc = C.untyped_storage().nbytes() // 4
    oc = (d.C - C.untyped_storage().data_ptr()) // 4
    out = [float('nan')] * nc
    written = set()

    def at(flat, idx, what):
        assert 0 <= idx < len(flat), f'{what}: element {idx} outside a storage of {len(flat)}'
        return flat[idx]

    nb = [max(int(n), 1) for n in d.nb]
    for i0, i1, i2 in itertools.product(range(nb[0]), range(nb[1]), range(nb[2])):
        a0 = oa + i0 * d.sA[0] + i1 * d.sA[1] + i2 * d.sA[2]
        b0 = ob + i0 * d.sB[0] + i1 * d.sB[1] + i2 * d.sB[2]
        c0 = oc + i0 * d.sC[0] + i1 * d.sC[1] + i2 * d.sC[2]
        d0 = od + i0 * d.sD[0] + i1 * d.sD[1] + i2 * d.sD[2]
        for row in range(d.M):
            for col in range(d.N):
                acc = 0.0
                for k in range(d.K):
                    a = at(fa, a0 + (k * d.lda + row if d.transA else row * d.lda + k), 'A')
                    b = at(fb, b0 + (col * d.ldb + k if d.transB else k * d.ldb + col), 'B')
                    acc += a * b
                v = d.alpha * acc
                if d.D:
                    v += d.beta * at(fd, d0 + row * d.ldd + col, 'D')
                ic = c0 + row * d.ldc + col
                assert 0 <= ic < nc, f'C: element {ic} outside a storage of {nc}'
                assert ic not in written, f'C: element {ic} written twice'
                written.add(ic)
                out[ic] = v
    return torch.tensor(out, dtype=torch.float64)


def run(A, B, D=None, out=None, tri=(0, 0, 0)):
    """build the descriptor, interpret it, compare with fp64; -> (desc, keep)"""
    bshape = torch.broadcast_shapes(A.shape[:-2], B.shape[:-2], D.shape[:-2] if D is not None else ())
    d, keep, Cr = ops._gemm_desc(A, B, D, out, ALPHA, BETA, *tri)
    C = Cr if out is None else out
    assert Cr is C and tuple(C.shape) == (*bshape, A.shape[-2], B.shape[-1])
    assert (d.M, d.K, d.N) == (A.shape[-2], A.shape[-1], B.shape[-1]) and (d.alpha, d.beta) == (ALPHA, BETA)
    assert (d.triA, d.triB, d.triC) == tri and (d.D is None) == (D is None)
    assert d.lda >= 1 and d.ldb >= 1 and d.ldc >= 1
    store = interpret(d, keep, C)
    want = ALPHA * (A.double() @ B.double())
    if D is not None:
        want = want + BETA * D.double()
    got = torch.as_strided(store, C.shape, C.stride(), C.storage_offset())
    assert torch.equal(got, want.expand_as(got))
    assert int((~store.isnan()).sum()) == C.numel(), 'written outside the result'
    return d, keep


def in_place(d, which, view, trans, ld):
    """operand `which` is consumed where it lies: no copy, the expected layout"""
    assert getattr(d, which) == view.data_ptr()
    if which != 'D':
        assert getattr(d, 'trans' + which) == trans
    assert getattr(d, 'ld' + which.lower()) == ld


def test_contiguous():
    A, B, D = _ints((2, 3, 5, 7), 1), _ints((2, 3, 7, 4), 2), _ints((2, 3, 5, 4), 3)
    d, _ = run(A, B, D)
    in_place(d, 'A', A, 0, 7), in_place(d, 'B', B, 0, 4), in_place(d, 'D', D, 0, 4)
    assert list(d.nb) == [1, 2, 3] and list(d.sA) == [0, 105, 35] and list(d.sB) == [0, 84, 28]
    assert list(d.sC) == [0, 60, 20] and list(d.sD) == [0, 60, 20] and d.ldc == 4
    run(A, B)
    run(A, B, D, tri=(ops.LOWER, ops.UPPER, ops.NONE))


@pytest.mark.parametrize('tA,tB', [(0, 1), (1, 0), (1, 1)])
def test_transposed_views(tA, tB):
    A = _ints((2, 3, 7, 5), 4).mT if tA else _ints((2, 3, 5, 7), 4)
    B = _ints((3, 4, 7), 5).mT if tB else _ints((3, 7, 4), 5)
    d, _ = run(A, B, _ints((2, 3, 5, 4), 6))
    in_place(d, 'A', A, tA, 5 if tA else 7), in_place(d, 'B', B, tB, 7 if tB else 4)
    assert list(d.sB) == [0, 0, 28]


def test_row_padded_views():
    A = _ints((2, 3, 5, 10), 7)[..., :7]
    B = _ints((3, 7, 9), 8)[..., :4]
    D = _ints((2, 3, 5, 6), 9)[..., :4]
    d, _ = run(A, B, D)
    in_place(d, 'A', A, 0, 10), in_place(d, 'B', B, 0, 9), in_place(d, 'D', D, 0, 6)
    assert list(d.sA) == [0, 150, 50] and list(d.sD) == [0, 90, 30]
    At = _ints((2, 3, 7, 8), 10)[..., :5].mT            # (5 x 7) stored transposed with a padded leading dimension
    Bt = _ints((3, 4, 11), 11)[..., 2:9].mT             # ... and starting two elements into its rows
    d, _ = run(At, Bt, D)
    in_place(d, 'A', At, 1, 8), in_place(d, 'B', Bt, 1, 11)
    rows = _ints((2, 3, 9, 7), 12)[:, :, 2:7]           # a window of rows: no padding, but a batch stride larger than M K
    d, _ = run(rows, B)
    in_place(d, 'A', rows, 0, 7)
    assert list(d.sA) == [0, 189, 63]


def test_sliced_batch():
    A = _ints((4, 3, 5, 7), 13)[::2]
    B = _ints((2, 6, 7, 4), 14)[:, 1::2]
    D = _ints((5, 3, 5, 4), 15)[1:4:2]
    d, _ = run(A, B, D)
    in_place(d, 'A', A, 0, 7), in_place(d, 'B', B, 0, 4), in_place(d, 'D', D, 0, 4)
    assert list(d.sA) == [0, 210, 35] and list(d.sB) == [0, 168, 56] and list(d.sD) == [0, 120, 20]


def test_stride0_batch():
    A, B, D = _ints((3, 5, 7), 16), _ints((2, 1, 7, 4), 17), _ints((1, 3, 5, 4), 18)
    d, _ = run(A, B, D)
    in_place(d, 'A', A, 0, 7), in_place(d, 'B', B, 0, 4), in_place(d, 'D', D, 0, 4)
    assert list(d.sA) == [0, 0, 35] and list(d.sB) == [0, 28, 0] and list(d.sD) == [0, 0, 20]
    Ax = _ints((1, 5, 7), 19).expand(3, 5, 7)           # an explicit expand, and a transposed view of one
    d, _ = run(Ax, B, D)
    in_place(d, 'A', Ax, 0, 7)
    assert list(d.sA) == [0, 0, 0]
    d, _ = run(_ints((1, 7, 5), 20).expand(3, 7, 5).mT, B, D)
    assert d.transA == 1 and d.lda == 5 and list(d.sA) == [0, 0, 0]


@pytest.mark.parametrize('dshape', [(1, 4), (5, 1), (1, 1), (3, 1, 4), (2, 1, 5, 1), (1, 3, 1, 1), (4,), (2, 3, 1, 4)])
def test_broadcast_d(dshape):
    """D broadcast over rows (stride(-2) == 0: the kernel's `row * ldd + col` cannot express it, so it has to be
    materialised), over columns, over both, with and without batch dimensions."""
    run(_ints((2, 3, 5, 7), 21), _ints((3, 7, 4), 22), _ints(dshape, 23))


def test_broadcast_d_one_column_and_one_row():
    A = _ints((2, 3, 5, 7), 24)
    run(A, _ints((3, 7, 1), 25), _ints((1, 1), 26))              # N == 1, D one element for all rows
    run(A, _ints((3, 7, 1), 25), _ints((3, 5, 1), 27))
    run(A[:, :, :1], _ints((3, 7, 4), 28), _ints((1, 4), 29))    # M == 1: a row-broadcast D is the row itself
    d, _ = run(A, _ints((3, 7, 1), 25), _ints((2, 3, 5, 3), 30)[..., 1:2])   # N == 1, a column of a wider D, in place
    assert d.ldd == 3


def test_two_dimensional_operands_against_a_batch():
    A, D = _ints((5, 7), 31), _ints((5, 4), 32)
    d, _ = run(A, _ints((2, 3, 7, 4), 33), D)
    in_place(d, 'A', A, 0, 7), in_place(d, 'D', D, 0, 4)
    assert list(d.nb) == [1, 2, 3] and list(d.sA) == [0, 0, 0] and list(d.sD) == [0, 0, 0]
    run(A, _ints((2, 2, 1, 3, 7, 4), 34), D)                     # four batch dimensions: the operands are folded into one
    run(A.mT.contiguous().mT, _ints((2, 2, 1, 3, 4, 7), 35).mT, _ints((1, 4), 36))


def test_more_than_three_batch_dimensions():
    A, B = _ints((2, 1, 2, 3, 5, 7), 37), _ints((2, 2, 1, 7, 4), 38)
    d, _ = run(A, B, _ints((2, 1, 3, 5, 4), 39))
    assert list(d.nb) == [1, 1, 24]
    run(A, B.mT.contiguous().mT, _ints((3, 1, 4), 40))
    run(_ints((2, 2, 2, 3, 5, 7), 41), B)                        # A folds without a copy
    out = torch.full((2, 2, 2, 3, 5, 6), float('nan'))[..., :4]  # padded rows: the batch dimensions still fold into one
    d, _ = run(A, B, out=out)
    assert d.ldc == 6 and d.C == out.data_ptr()
    out = torch.full((2, 2, 2, 4, 5, 4), float('nan'))[:, :, :, :3]
    with pytest.raises(RuntimeError):                            # ... here they do not: an error, not a product written to a copy
        ops._gemm_desc(A, B, None, out, 1.0, 0.0, 0, 0, 0)


@pytest.mark.parametrize('M,N,K', [(1, 4, 7), (5, 1, 7), (5, 4, 1), (1, 1, 7), (1, 4, 1), (5, 1, 1), (1, 1, 1)])
def test_unit_sizes(M, N, K):
    for tA, tB in itertools.product((0, 1), (0, 1)):
        A = _ints((2, 3, K, M), 42).mT if tA else _ints((2, 3, M, K), 42)
        B = _ints((3, N, K), 43).mT if tB else _ints((3, K, N), 43)
        run(A, B, _ints((2, 3, M, N), 44))
    run(_ints((2, 3, M, K + 2), 45)[..., 1:K + 1], _ints((3, K + 1, N + 3), 46)[:, :K, 2:N + 2], _ints((3, 1, N), 47))
    run(_ints((2, 3, M, 3 * K), 48)[..., ::3], _ints((3, K, 2 * N), 49)[..., ::2], _ints((M, 1), 50))


def test_storage_offset_of_one_element():
    """Views that start one element into their storage: 4-byte aligned only, and still consumed in place."""
    A, B, D = _ints((2, 3, 5, 7), 51, offset=1), _ints((3, 4, 7), 52, offset=1).mT, _ints((3, 5, 4), 53, offset=1)
    assert A.storage_offset() == 1 and B.storage_offset() == 1 and D.storage_offset() == 1
    d, _ = run(A, B, D)
    in_place(d, 'A', A, 0, 7), in_place(d, 'B', B, 1, 7), in_place(d, 'D', D, 0, 4)
    out = torch.full((1 + 2 * 3 * 5 * 4,), float('nan'))[1:].view(2, 3, 5, 4)
    d, _ = run(A, B, D, out=out)
    assert d.C == out.data_ptr()


def test_out_is_a_window_of_a_larger_buffer():
    A, B, D = _ints((2, 3, 5, 7), 54), _ints((3, 7, 4), 55), _ints((2, 1, 5, 4), 56)
    buf = torch.full((2, 3, 8, 9), float('nan'))
    out = buf[:, :, 1:6, 2:6]
    d, _ = run(A, B, D, out=out)
    assert d.C == out.data_ptr() and d.ldc == 9 and list(d.sC) == [0, 216, 72]
    out = torch.full((4, 3, 5, 9), float('nan'))[1::2, :, :, 5:]          # every other batch entry
    d, _ = run(A, B, out=out)
    assert list(d.sC) == [0, 270, 45]
    col = torch.full((2, 3, 5, 6), float('nan'))[..., 2:3]                # N == 1: one column of a wider buffer
    d, _ = run(A, _ints((3, 7, 1), 57), out=col)
    assert d.ldc == 6
    with pytest.raises(AssertionError):
        ops._gemm_desc(A, B, None, torch.empty(2, 3, 4, 5).mT, 1.0, 0.0, 0, 0, 0)   # columns of C are not contiguous
