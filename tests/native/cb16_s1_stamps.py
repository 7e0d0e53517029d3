"""Inside S1 of the blocked pivot chain (csrc/chol_blk16.h; a -DVARGP_CB16_STAMPS build of chol.hip): cycles of the owner wave
of each step from S1's start to the block in column layout, to the end of the sixteen pivots, to the E / ED stores issued, and
to the far side of B1; then the whole step and the chain.
VARGP_HIP_LIB=<that .so> VARGP_CHOL_F32_ALONE=1 python tests/native/cb16_s1_stamps.py"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
from vargp_amd import _lib, ops  # noqa: E402
ops.set_cholesky_error_mode('defer')
A = torch.randn(30, 100, 100, device='cuda')
A = A @ A.mT / 100 + torch.eye(100, device='cuda')
for _ in range(3):
    ops.chol_inv(A)
torch.cuda.synchronize()
dll = ctypes.CDLL(_lib.LIB_PATH)
buf, b1 = (ctypes.c_ulonglong * 128)(), (ctypes.c_ulonglong * 32)()
dll.vargp_debug_cb16_stamps(buf)
dll.vargp_debug_cb16_s1_stamps(b1)
t = [[[buf[(w * 8 + s) * 4 + i] for i in range(4)] for s in range(8)] for w in range(4)]
owner = lambda k: 6 - k if k >= 3 else k + 1
tot = [0, 0, 0, 0, 0]
for k in range(7):
    w = owner(k)
    s0 = t[w][k][0]
    lay, piv, out, bar = b1[k * 4] - s0, b1[k * 4 + 1] - b1[k * 4], b1[k * 4 + 2] - b1[k * 4 + 1], t[w][k][1] - b1[k * 4 + 2]
    step = (t[w][k + 1][0] if k < 6 else t[w][7][0]) - s0
    for i, x in enumerate((lay, piv, out, bar, step)):
        tot[i] += x
    print('step %d (wave %d): layout %5d  pivots %5d  scale + write-out %5d  to behind B1 %5d | S1 %5d  step %5d' % (
        k, w, lay, piv, out, bar, lay + piv + out + bar, step))
print('sum            : layout %5d  pivots %5d  scale + write-out %5d  to behind B1 %5d | S1 %5d  steps %5d' % (
    *tot[:4], sum(tot[:4]), tot[4]))
t0 = min(t[w][0][0] for w in range(4) if t[w][0][0])
print('chain: last S3 done @%d, end barrier reached @%s, written @%s' % (
    max(t[w][6][3] for w in range(4)) - t0, [t[w][7][0] - t0 for w in range(4)], [t[w][7][1] - t0 for w in range(4)]))
