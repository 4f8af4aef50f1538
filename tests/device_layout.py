"""Device buffers laid out the way a caller of the `_dev` entry points may hold them (include/elfihip.h: the `_dev` layout
contract): rows at a pitch that is not the width, a base that is only 8-byte aligned, results next to other data.

`place` surrounds the rows with NaN, so a kernel that reads with the wrong pitch or offset returns NaN instead of a
plausible number; `guarded_out` surrounds the results with a sentinel, so a store outside them (a 16-byte store that
straddles the end, a row too many) is seen.  A plain module: the GPU tests import it, it defines no fixture.
"""
import numpy as np

# (ldx - m, off) in doubles.  A torch allocation starts on a 16-byte boundary (checked below), so `off` even keeps row 0
# 16-byte aligned and `ldx` even keeps every later row so: with m even those are the layouts of the 16-byte-load paths.
LAYOUTS = [(0, 0), (2, 0), (6, 2), (1, 0), (0, 1), (3, 1)]
PACKED = (0, 0)

SENTINEL = -7.0625e300            # never a distance, a mean of the test data, or a variance
_LEAD = 2                         # doubles in front of every output buffer (keeps the parity of `off`)
_TAIL = 8


def vec2(m, layout):
    """make_row_args' condition for 16-byte row loads: m even, ldx even, 16-byte aligned base."""
    pad, off = layout
    return m % 2 == 0 and (m + pad) % 2 == 0 and off % 2 == 0


def place(X, ldx, off):
    """Host (n, m) float64 matrix -> 1-d device buffer with row r at element off + r * ldx; every other element (lead-in,
    gap columns, one pitch of tail) is NaN.  Returns (tensor, address of row 0); the tensor keeps the memory alive."""
    import torch
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, m = X.shape
    assert ldx >= m and off >= 0
    host = np.full(off + n * ldx + ldx, np.nan)
    rows = np.lib.stride_tricks.as_strided(host[off:], shape=(n, m), strides=(8 * ldx, 8))
    rows[...] = X
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 8 * off


def place_rows_only(X, ldx, off):
    """As `place` for pitches too large to fill: the buffer is torch.empty, only the n rows are written."""
    import torch
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, m = X.shape
    t = torch.empty(off + (n - 1) * ldx + m, dtype=torch.float64, device='cuda')
    assert t.data_ptr() % 16 == 0
    torch.as_strided(t, (n, m), (ldx, 1), off).copy_(torch.from_numpy(X).cuda())
    return t, t.data_ptr() + 8 * off


def to_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


class GuardedOut:
    """n x K results at element `off` of a buffer that is SENTINEL everywhere (the results included: a result that was
    never written is seen too)."""

    def __init__(self, n, K=1, off=0):
        import torch
        self.n, self.K, self.start = n, K, _LEAD + off
        self.t = torch.full((self.start + n * K + _TAIL,), SENTINEL, dtype=torch.float64, device='cuda')
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 8 * self.start

    def check(self):
        """The sentinels in front of and behind the results are untouched and every result was written -> (n, K) array
        ((n,) for K = 1).  The caller has synchronised the stream that wrote."""
        h = self.t.cpu().numpy()
        s, e = self.start, self.start + self.n * self.K
        guard = np.float64(SENTINEL).view(np.int64)
        assert np.all(h[:s].view(np.int64) == guard), 'store in front of the results'
        assert np.all(h[e:].view(np.int64) == guard), 'store behind the results'
        res = h[s:e].copy()
        assert not np.any(res.view(np.int64) == guard), 'a result was not written'
        return res if self.K == 1 else res.reshape(self.n, self.K)


def guarded_out(n, K=1, off=0):
    return GuardedOut(n, K, off)
