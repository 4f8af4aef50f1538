"""The sampler state's merge inside the next distance pass (reject.hip, dist_rows_dma_kernel<..., MERGE>).

At a merge point a row push seals its candidate list; the next row push of the DMA form (m = 16 / 32 / 64) merges it in
one workgroup of its own launch, and every other reader of the state merges it first.  These tests run long push
sequences WITHOUT result() in between (so the merge cadence reaches its 8-push interval and lists are sealed), with
flush / result / state_dev / export swaps / reset / other push forms inserted at points where a list may be sealed, and
compare the state with NumPy's lexsort top-k bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _topk(d, rows, k):
    ok = ~np.isnan(d)                                  # a NaN never enters the state
    d, rows = d[ok], rows[ok]
    order = np.lexsort((rows, d))[:k]
    return d[order], rows[order]


class _Seq:
    """One device state, its pushes, and the reference state kept beside it."""

    def __init__(self, hip_ctx, k, m, seed):
        import torch
        self.torch, self.ctx, self.lib, self.k, self.m = torch, hip_ctx, hip_ctx.lib, k, m
        self.h = C.c_void_p()
        hip_ctx.call("elfihip_reject_create", k, C.byref(self.h))
        rs = np.random.RandomState(seed)
        self.rs = rs
        self.yh = rs.randn(1, m)
        self.y = torch.from_numpy(self.yh).cuda()
        self.exp = [torch.empty(2 * k, dtype=torch.float64, device="cuda") for _ in range(2)]
        self.cur = 0
        self.base = 0
        self.ref_d = np.empty(0)
        self.ref_r = np.empty(0, dtype=np.int64)
        self.pending = []                               # (device distances, rows) not yet folded into the reference

    def batch(self, n):
        """A device batch with NaN, +-inf and rows equal to y (distance 0: ties), and duplicated rows (ties)."""
        X = self.rs.randn(n, self.m)
        X[5::997] = np.nan
        X[7::1999, 3] = np.inf
        X[11::2003, 1] = -np.inf
        X[13::4001] = self.yh
        X[200:300] = X[100:200]
        return self.torch.from_numpy(X).cuda()

    def _fold(self):
        if not self.pending:
            return
        self.ctx.synchronize()
        d = np.concatenate([self.ref_d] + [o.cpu().numpy() for o, _ in self.pending])
        r = np.concatenate([self.ref_r] + [rr for _, rr in self.pending])
        self.ref_d, self.ref_r = _topk(d, r, self.k)
        self.pending = []

    def push_rows(self, X):
        torch = self.torch
        n = X.shape[0]
        out = torch.empty(n, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        self.export_swap()
        assert self.lib.elfihip_reject_push_rows_dev(self.h, 0, X.data_ptr(), n, self.m, self.m, self.y.data_ptr(), None,
                                                     2.0, out.data_ptr(), self.base) == 0
        self.pending.append((out, self.base + np.arange(n, dtype=np.int64)))
        self.base += n + 7919                          # increasing global row numbers, with gaps
        if len(self.pending) >= 8:
            self._fold()
        return out

    def push_dev(self, src, n, scale):
        """Distances that exist already (no DMA row pass: the sealed list takes the standalone merge)."""
        self.ctx.synchronize()
        d = src[:n] * scale
        self.torch.cuda.synchronize()
        assert self.lib.elfihip_reject_push_dev(self.h, d.data_ptr(), n, 1, self.base) == 0
        self.pending.append((d.clone(), self.base + np.arange(n, dtype=np.int64)))
        self.base += n + 7919

    def export_swap(self):
        self.cur ^= 1
        assert self.lib.elfihip_reject_export_dev(self.h, self.exp[self.cur].data_ptr()) == 0

    def check_result(self):
        self._fold()
        k = self.k
        vals, rows, cnt = np.empty(k), np.empty(k, dtype=np.int64), C.c_int64()
        assert self.lib.elfihip_reject_result(self.h, vals.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                                              C.byref(cnt)) == 0          # (an overflowed list fails here)
        c = cnt.value
        assert c == len(self.ref_d)
        assert np.array_equal(vals[:c], self.ref_d) and np.array_equal(rows[:c], self.ref_r)
        return vals, rows

    def check_export(self):
        """The export buffer current now holds the state (after a flush / state_dev)."""
        self._fold()
        self.ctx.synchronize()
        e = self.exp[self.cur]
        c = len(self.ref_d)
        ev = e[:self.k].cpu().numpy()[:c]
        er = e[self.k:].view(self.torch.int64).cpu().numpy()[:c]
        assert np.array_equal(ev, self.ref_d) and np.array_equal(er, self.ref_r)

    def flush(self):
        assert self.lib.elfihip_reject_flush(self.h) == 0
        self.check_export()

    def state_dev(self):
        pv, pr = C.c_void_p(), C.c_void_p()
        assert self.lib.elfihip_reject_state_dev(self.h, C.byref(pv), C.byref(pr)) == 0
        assert pv.value and pr.value
        self.check_export()

    def reset(self):
        assert self.lib.elfihip_reject_reset(self.h) == 0
        self.pending = []
        self.ref_d = np.empty(0)
        self.ref_r = np.empty(0, dtype=np.int64)

    def free(self):
        self.lib.elfihip_reject_free(self.h)


@pytest.mark.parametrize("m", [16, 32, 64])
@pytest.mark.parametrize("k", [1, 64, 1000, 1024, 1025, 2048])
def test_fused_merge_long_sequences(hip_ctx, m, k):
    """44 pushes of 10^5 - 10^6 rows from three batches in rotation (repeated under new row numbers); flush, result,
    state_dev, a push of existing distances and a reset in between.  k <= 1024 takes the fused merge, k > 1024 the
    standalone one."""
    S = _Seq(hip_ctx, k, m, seed=1000 * m + k)
    Xs = [S.batch(100000), S.batch(100000), S.batch(1000000)]
    events = {9: "flush", 14: "result", 19: "state_dev", 23: "push_dev", 27: "flush", 31: "reset", 36: "state_dev"}
    last = None
    for i in range(44):
        last = S.push_rows(Xs[i % 3])
        ev = events.get(i)
        if ev == "flush":
            S.flush()
        elif ev == "result":
            S.check_result()
        elif ev == "state_dev":
            S.state_dev()
        elif ev == "push_dev":
            S.push_dev(last, 50000, 0.5)               # rows that beat most of the state
        elif ev == "reset":
            S.check_result()
            S.reset()
    S.check_result()
    S.flush()
    S.free()


@pytest.mark.parametrize("small", [10, 11])
def test_fused_merge_select_push_in_the_middle(hip_ctx, small):
    """Small pushes, then one whose expected candidates take the radix selection (n k / rows seen > 8192) -- after 10
    pushes a list is sealed, after 11 none -- then long filtered sequences again."""
    k, m = 1000, 32
    S = _Seq(hip_ctx, k, m, seed=77 + small)
    Xa = S.batch(5000)
    Xb = S.batch(1000000)
    Xc = S.batch(200000)
    for _ in range(small):
        S.push_rows(Xa)
    S.push_rows(Xb)                                   # 10^6 x 1000 / (5 10^4 or 5.5 10^4) > 8192: selection
    for i in range(40):
        S.push_rows(Xc if i % 2 else Xb)
        if i == 20:
            S.export_swap()
            S.flush()
    S.check_result()
    S.free()


def test_fused_merge_matches_separate_reads_of_the_same_sequence(hip_ctx):
    """Two states fed the same 41 pushes: one read after every push (each read merges everything, no list is ever
    sealed), one only at the end -- the same state, the same export."""
    k, m = 1000, 64
    A = _Seq(hip_ctx, k, m, seed=5)
    B = _Seq(hip_ctx, k, m, seed=5)
    Xs = [A.batch(300000), A.batch(300000)]
    for i in range(41):
        A.push_rows(Xs[i % 2])
        B.push_rows(Xs[i % 2])
        A.check_result()
    va, ra = A.check_result()
    vb, rb = B.check_result()
    assert np.array_equal(va, vb) and np.array_equal(ra, rb)
    A.free()
    B.free()
