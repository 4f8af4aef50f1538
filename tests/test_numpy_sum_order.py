"""The summation order elfi_amd/csrc/np_sum.hpp restates, held against NumPy itself: pairwise inside pieces of the
reduction's buffer (8192 elements), the pieces added in order.  The row summaries and the fused Gaussian kernel are
bit-identical to np.mean / np.var only while this model is; if a NumPy release changes the order, this test says so
without a GPU."""
import numpy as np
import pytest

BUFSIZE = 8192      # np_sum.hpp: NP_BUFSIZE


def pairwise(x):
    """NumPy's pairwise_sum along the rows of x (n, L), as np_pairwise does it."""
    n, L = x.shape
    if L < 8:
        r = np.zeros(n)
        for i in range(L):
            r = r + x[:, i]
        return r
    if L <= 128:
        r = [x[:, j].copy() for j in range(8)]
        i = 8
        while i < L - L % 8:
            for j in range(8):
                r[j] = r[j] + x[:, i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for k in range(i, L):
            res = res + x[:, k]
        return res
    n2 = L // 2
    n2 -= n2 % 8
    return pairwise(x[:, :n2]) + pairwise(x[:, n2:])


def row_sum(x):
    """np_pairwise_row."""
    acc = pairwise(x[:, :BUFSIZE])
    for lo in range(BUFSIZE, x.shape[1], BUFSIZE):
        acc = acc + pairwise(x[:, lo:lo + BUFSIZE])
    return acc


@pytest.mark.parametrize('L', [1, 7, 8, 129, 1003, 8192, 8193, 16385, 20479, 30000])
def test_row_reduction_is_pairwise_in_pieces_of_the_buffer(L):
    assert np.getbufsize() == BUFSIZE
    rs = np.random.RandomState(L)
    for n in (1, 5):
        x = rs.randn(n, L) * 3 + 1
        assert np.array_equal(np.add.reduce(x, axis=1), row_sum(x)), (n, L)
        assert np.array_equal(np.mean(x, axis=1), row_sum(x) / L), (n, L)
        d = x - np.mean(x, axis=1, keepdims=True)
        assert np.array_equal(np.var(x, axis=1), row_sum(d * d) / L), (n, L)


def test_the_pieces_matter_beyond_one_buffer():
    """The plain recursion over the whole row is another number from 8193 terms on: what the long-row GPU tests catch."""
    x = np.random.RandomState(0).randn(64, 20479) * 3 + 1
    assert not np.array_equal(pairwise(x), row_sum(x))
