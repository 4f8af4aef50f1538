"""GPU: Gaussian-mixture proposal density vs the reference's GMDistribution (golden fixture from the
real class) and the oracle.  Tolerance 1e-12 relative: same factorisation of the covariance and same
accumulation order as the reference; the device exp() differs from libm's in the last bits."""
import os

import numpy as np
import pytest

import gm_oracle as GM
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def test_against_the_reference_class(hip_ctx):
    import elfi_amd
    g = np.load(os.path.join(GOLDEN, 'gm_pdf.npz'))
    for k in g['cases']:
        x, means, w = g['x_%d' % k], g['means_%d' % k], g['w_%d' % k]
        cov = g['cov_%d' % k]
        cov = float(cov) if cov.ndim == 0 else cov
        got = elfi_amd.GMDistribution.pdf(x, means, cov=cov, weights=w)
        np.testing.assert_allclose(got, g['pdf_%d' % k], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(elfi_amd.GMDistribution.logpdf(x, means, cov=cov, weights=w), g['logpdf_%d' % k],
                                   rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(elfi_amd.GMDistribution.pdf(x, means, cov=cov), g['pdf_now_%d' % k], rtol=1e-12,
                                   atol=1e-300)
    single = elfi_amd.GMDistribution.pdf(g['x_1'][3], g['means_1'], cov=g['cov_1'], weights=g['w_1'])
    assert np.ndim(single) == 0 and single == pytest.approx(float(g['pdf_single']), rel=1e-12)


@pytest.mark.parametrize('M,N,d', [(1, 1, 1), (1000, 1000, 2), (5000, 257, 4), (300, 2000, 8), (77, 50, 16)])
def test_vs_oracle(hip_ctx, M, N, d):
    import elfi_amd
    rs = np.random.RandomState(M + N + d)
    means = rs.randn(N, d)
    x = rs.randn(M, d) * 1.5
    A = rs.randn(d, d)
    cov = (A @ A.T + d * np.eye(d)) / (3.0 * d)
    w = rs.uniform(0.5, 1.5, N)
    got = elfi_amd.GMDistribution.pdf(x, means, cov=cov, weights=w)
    np.testing.assert_allclose(got, GM.pdf(x, means, cov=cov, weights=w), rtol=1e-12, atol=1e-300)
    got = elfi_amd.GMDistribution.pdf(x, means, cov=0.37)              # scalar covariance, unit weights
    np.testing.assert_allclose(got, GM.pdf(x, means, cov=0.37), rtol=1e-12, atol=1e-300)


def test_errors(hip_ctx):
    import elfi_amd
    with pytest.raises(ValueError):
        elfi_amd.GMDistribution.pdf(np.zeros((3, 2)), np.zeros((4, 3)))
    with pytest.raises(np.linalg.LinAlgError):
        elfi_amd.GMDistribution.pdf(np.zeros((3, 2)), np.zeros((4, 2)), cov=np.ones((2, 2)))
    with pytest.raises(NotImplementedError):
        elfi_amd.GMDistribution.pdf(np.zeros((3, 65)), np.zeros((4, 65)))


@pytest.mark.parametrize('d', [17, 20, 32, 33, 64])
def test_many_parameters(hip_ctx, d):
    """16 < d <= 64: both point sets are transformed by the covariance factor once, a pair then costs d subtractions."""
    import elfi_amd
    import gm_oracle as GM
    rs = np.random.RandomState(d)
    M, N = 777, 300
    x, means = rs.randn(M, d), rs.randn(N, d) * 0.8
    A = rs.randn(d, d)
    cov = A @ A.T / d + 0.5 * np.eye(d)
    w = rs.uniform(0.5, 1.5, N)
    ref = GM.pdf(x, means, cov=cov, weights=w)
    np.testing.assert_allclose(elfi_amd.GMDistribution.pdf(x, means, cov=cov, weights=w), ref, rtol=1e-11, atol=1e-300)
    np.testing.assert_allclose(elfi_amd.GMDistribution.logpdf(x, means, cov=cov, weights=w), np.log(ref), rtol=1e-11, atol=1e-11)


def test_rvs_on_the_device_has_the_mixtures_moments(hip_ctx):
    """GMDistribution.rvs (elfi/methods/utils.py:199-262) on the device: shapes as the reference's, components by their
    weights, perturbations with the shared covariance, the validity loop against the prior; seeded by the RandomState."""
    from elfi_amd import GMDistribution
    rs = np.random.RandomState(0)
    N, d, n = 7, 3, 400000
    means = rs.uniform(-5, 5, (N, d))
    w = rs.uniform(0.1, 1.0, N)
    w[2] = 0.0                                     # a component without mass is never drawn
    B = rs.randn(d, d)
    cov = B @ B.T / d + 0.1 * np.eye(d)
    x = GMDistribution.rvs(means, cov, w, size=n, random_state=np.random.RandomState(5))
    assert x.shape == (n, d)
    assert np.array_equal(x, GMDistribution.rvs(means, cov, w, size=n, random_state=np.random.RandomState(5)))
    assert not np.array_equal(x, GMDistribution.rvs(means, cov, w, size=n, random_state=np.random.RandomState(6)))
    wn = w / w.sum()
    m_true = wn @ means
    c_true = cov + (means - m_true).T @ np.diag(wn) @ (means - m_true)
    assert np.max(np.abs(x.mean(axis=0) - m_true)) < 5 * np.sqrt(np.max(np.diag(c_true)) / n) + 1e-12
    assert np.max(np.abs(np.cov(x.T) - c_true)) < 0.02 * np.max(np.abs(c_true))
    # well separated components: the shares of the draws are the weights, a component without mass is never drawn
    far = 100.0 * np.arange(N)[:, None] * np.ones((1, d))
    xf = GMDistribution.rvs(far, 0.01 * np.eye(d), w, size=n, random_state=np.random.RandomState(7))
    comp = np.rint(xf[:, 0] / 100.0).astype(int)
    share = np.bincount(comp, minlength=N) / n
    assert share[2] == 0.0
    assert np.max(np.abs(share - wn)) < 5 * np.sqrt(0.25 / n)
    # 1-d means, scalar covariance, size None / int
    m1 = np.array([-2.0, 0.5, 3.0])
    y = GMDistribution.rvs(m1, 0.25, None, size=200000, random_state=np.random.RandomState(1))
    assert y.shape == (200000,)
    assert abs(y.mean() - m1.mean()) < 0.02 and abs(y.var() - (0.25 + m1.var())) < 0.05
    one = GMDistribution.rvs(m1, 0.25, None, size=None, random_state=np.random.RandomState(1))
    assert np.ndim(one) == 0
    # the validity loop: only points the prior accepts come back, still `size` of them
    logp = lambda v: np.where(v > 0.0, 0.0, -np.inf)     # noqa: E731
    z = GMDistribution.rvs(m1, 0.25, None, size=50000, prior_logpdf=logp, random_state=np.random.RandomState(2))
    assert z.shape == (50000,) and np.all(z > 0.0)
    with pytest.raises(ValueError):
        GMDistribution.rvs(means, np.eye(2), w, size=3)


# ---- every mixture draw against the model of gm_rvs_kernel (csrc/gmix.hip) ---------------------------------------------
# Draw i of (seed, stream) is a pure function of its index: the component by inverse CDF from the first 53-bit word of
# Philox counter i (tests/philox_ref.py), the perturbation A z_i from normals i ceil(d / 2) ... of stream + 1, which are
# the numbers elfihip_randn_dev writes.  gmix.hip lets the compiler contract a product and a sum into an FMA, so the
# values are held to the summation bound of d + 1 terms instead of bits: (d + 2) 2^-53 (|mean_a| + sum_c |A_ac z_c|).

GM_SEED, GM_STREAM = (0x1234 << 32) | 0x9abcdef1, (7 << 32) | 5      # the high key and counter words are used
FAR = 1000.0                                                          # spacing of the well separated means


def _gm_call(ctx, seed, stream, n, means, cumw, A):
    import ctypes as C
    from elfi_amd import _lib
    means, cumw, A = (np.ascontiguousarray(a, dtype=np.float64) for a in (means, cumw, A))
    N, d = means.shape
    assert cumw.shape == (N,) and A.shape == (d, d)
    x = np.full((n, d), np.nan)
    ctx.call('elfihip_gm_rvs', C.c_uint64(seed), C.c_uint64(stream), n, d, _lib.ptr(means), N, _lib.ptr(cumw), _lib.ptr(A),
             _lib.ptr(x))
    return x


def _gm_normals(ctx, seed, stream, n, d):
    """z_i: row i of the (n, 2 ceil(d / 2)) matrix of the stream after the components', first d columns."""
    import ctypes as C
    import torch
    w = 2 * ((d + 1) // 2)
    t = torch.empty(n * w, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    ctx.call('elfihip_randn_dev', C.c_uint64(seed), C.c_uint64(stream + 1), n * w, C.c_double(0.0), C.c_double(1.0), t.data_ptr())
    ctx.synchronize()
    return t.cpu().numpy().reshape(n, w)[:, :d].copy()


def _gm_components(seed, stream, n, cumw):
    import philox_ref
    u = philox_ref.uniform53_first(seed, stream, np.arange(n, dtype=np.uint64))
    return np.minimum(np.searchsorted(cumw, u, side='right'), len(cumw) - 1), u


def _two_product(a, b):
    """a * b = p + e exactly (Dekker's product on Veltkamp's split; no overflow at the tests' magnitudes)."""
    p = a * b

    def split(v):
        c = 134217729.0 * v
        hi = c - (c - v)
        return hi, v - hi
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _affine_ref(mean_rows, A, z):
    """mean + A z per draw and the sum of the magnitudes of its d + 1 terms, beyond binary64: accumulated in np.longdouble
    where that has a 64-bit significand, else math.fsum over the exact products -> (ref, mag) as (n, d) arrays."""
    n, d = z.shape
    if np.finfo(np.longdouble).nmant >= 63:
        ld = np.longdouble
        ref, mag = mean_rows.astype(ld), np.abs(mean_rows).astype(ld)
        Al, zl = A.astype(ld), z.astype(ld)
        for c in range(d):
            t = zl[:, c, None] * Al[None, :, c]
            ref += t
            mag += np.abs(t)
        return ref, mag
    import math
    p, e = _two_product(z[:, None, :], A[None, :, :])                 # (n, a, c)
    ref, mag = np.empty((n, d)), np.empty((n, d))
    for i in range(n):
        for a in range(d):
            ref[i, a] = math.fsum([mean_rows[i, a]] + list(p[i, a]) + list(e[i, a]))
            mag[i, a] = math.fsum([abs(mean_rows[i, a])] + list(np.abs(p[i, a])) + list(np.abs(e[i, a])))
    return ref, mag


def _check_draws(ctx, seed, stream, n, means, cumw, A, never=()):
    """All n draws against the model: the component exactly (read off a first coordinate moved FAR apart per component)
    and every coordinate within the summation bound around the model's component.  -> (x, components)."""
    means = np.ascontiguousarray(means, dtype=np.float64)
    N, d = means.shape
    comp, u = _gm_components(seed, stream, n, cumw)
    z = _gm_normals(ctx, seed, stream, n, d)
    x = _gm_call(ctx, seed, stream, n, means, cumw, A)
    ref, mag = _affine_ref(means[comp], A, z)
    err = np.abs(x.astype(ref.dtype) - ref)
    bound = (d + 2) * 2.0 ** -53 * mag
    assert np.all(err <= bound), (d, N, n, float(np.max(err / mag)) * 2.0 ** 53)
    # the component on its own: |A z|_0 stays far below FAR / 2
    far = means.copy()
    far[:, 0] = FAR * np.arange(N) + means[:, 0]
    assert np.max(np.abs(means[:, 0])) + np.max(np.abs(z) @ np.abs(A[0])) < FAR / 4
    xf = _gm_call(ctx, seed, stream, n, far, cumw, A)
    got = np.rint(xf[:, 0] / FAR).astype(np.int64)
    assert np.array_equal(got, comp), (d, N, n)
    assert not np.isin(got, never).any()
    return x, comp, u


def _mixture(d, N, seed):
    rs = np.random.RandomState(seed)
    means = rs.uniform(-5, 5, (N, d))
    A = rs.randn(d, d) / d
    w = rs.uniform(0.1, 1.0, N)
    cumw = np.cumsum(w / w.sum())
    cumw[-1] = 1.0
    return means, cumw, A


@pytest.mark.parametrize('d,N', [(1, 1), (1, 3), (2, 7), (3, 7), (5, 1000), (64, 5)])
def test_rvs_every_draw_against_the_model(hip_ctx, d, N):
    """Odd d drops the second normal of the last pair, d = 1 has nothing else; N = 1 never searches; N = 1000 bisects ten
    times; d = 64 fills the kernel's z array."""
    n = 5000
    means, cumw, A = _mixture(d, N, 10 * d + N)
    x, comp, _ = _check_draws(hip_ctx, GM_SEED, GM_STREAM, n, means, cumw, A)
    # a prefix of a longer draw is the shorter draw
    assert np.array_equal(_gm_call(hip_ctx, GM_SEED, GM_STREAM, 1234, means, cumw, A), x[:1234])
    # seed and stream in the low words only: other numbers, the same model
    x2, _, _ = _check_draws(hip_ctx, 5, 3, n, means, cumw, A)
    assert not np.array_equal(x2, x)


def test_rvs_grid_stride_second_trip(hip_ctx):
    """The grid is at most 16 * cu_count blocks of 256: draws beyond that come from a second trip of the loop."""
    cu = hip_ctx.device_info()['cu_count']
    n = 256 * 16 * cu + 259
    means, cumw, A = _mixture(2, 7, 1)
    _check_draws(hip_ctx, GM_SEED, GM_STREAM, n, means, cumw, A)


def test_rvs_components_without_mass_and_the_clamp(hip_ctx):
    n, d, N = 5000, 3, 9
    means, _, A = _mixture(d, N, 2)
    # no mass in the first, a middle and the last component: cumw has ties (0 at the front, twice the same value inside,
    # 1 twice at the end), and the first index with cumw > u skips them
    w = np.random.RandomState(3).uniform(0.1, 1.0, N)
    w[[0, 4, N - 1]] = 0.0
    cumw = np.cumsum(w) / np.sum(w)
    cumw[N - 2:] = 1.0
    assert cumw[0] == 0.0 and cumw[4] == cumw[3] and cumw[N - 1] == cumw[N - 2] == 1.0
    _, comp, _ = _check_draws(hip_ctx, GM_SEED, GM_STREAM, n, means, cumw, A, never=(0, 4, N - 1))
    assert set(np.unique(comp)) == set(range(N)) - {0, 4, N - 1}
    # cumulative weights that end at 0.9: no entry exceeds u >= 0.9 and the search stops at N - 1 without reading past it
    cumw = np.linspace(0.1, 0.9, N)
    _, comp, u = _check_draws(hip_ctx, GM_SEED, GM_STREAM, n, means, cumw, A)
    clamped = u >= 0.9
    assert clamped.sum() > n // 20 and np.all(comp[clamped] == N - 1) and np.all(comp[u < 0.79] < N - 1)
