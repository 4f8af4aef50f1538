"""GPU: the wide Gaussian synthetic likelihood (csrc/synlik_wide.hip, 65 to 256 summaries) against a long-double truth
computed here, bit for bit against itself over prefixes, penalties, groups and the chunking of its launches, its edges and
the rejections of its two C entry points.

Bound of the parity test, the rule of tests/test_synlik.py (bound_for): 16 x the largest |float64 reference - truth| over
this test's cases and configurations of the same m (the reference is synlik_ref.syn_loglik_ref), floored at 16 ulp of
|truth|.
"""
import mpmath
import numpy as np
import pytest

import synlik_ref as R
from elfi_amd._lib import ERR_ARG

pytestmark = pytest.mark.gpu

LD = np.longdouble
PI = LD('3.14159265358979323846264338327950288')
# (seed, n, m, rho, smax): one column into the second 64-block, no multiple of 16, the scratch-assay width, n < m under
# shrinkage (S is singular: the Warton configurations only), the maximum
CASES = [(21, 80, 65, 0.8, 5.0), (22, 96, 80, 0.6, 8.0), (23, 170, 145, 0.7, 10.0), (24, 40, 145, 0.7, 10.0),
         (25, 300, 256, 0.8, 5.0)]
# ('unbiased' at the recipe's y has an indefinite psi at every one of these shapes, v' S^-1 v > n - 1: exactly -inf, from the
# truth too; 'unbiased-near' moves y to a fifth of its distance from the sample mean, where the estimator is finite)
CONFIGS = {'standard': {}, 'unbiased': dict(variant='unbiased'), 'unbiased-near': dict(variant='unbiased'),
           'warton0.1': dict(shrinkage='warton', penalty=0.1), 'warton0.8': dict(shrinkage='warton', penalty=0.8), 'whitening': 'W'}


def configs_of(n, m):
    return [k for k in CONFIGS if k.startswith('warton') or (n >= m + 2 and (not k.startswith('unbiased') or n > m + 3))]


def moments_ld(X):
    X = X.astype(LD)
    mean = X.sum(0) / len(X)
    D = X - mean
    return mean, D.T @ D / (len(X) - 1)


def chol_ld(S, v):
    """(log|S|, v^T S^-1 v) by a column Cholesky factorisation and the forward solve, in long double; None at a pivot
    that is not positive."""
    m = len(S)
    L = np.zeros((m, m), dtype=LD)
    z = np.zeros(m, dtype=LD)
    for j in range(m):
        col = S[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            return None
        L[j:, j] = col / np.sqrt(col[0])
        z[j] = (v[j] - L[j, :j] @ z[:j]) / L[j, j]
    return 2 * np.log(np.diag(L)).sum(), z @ z


def truth(X, y, variant='standard', shrinkage=None, penalty=None, whitening=None):
    X, y = X.astype(LD), y.astype(LD)
    if whitening is not None:
        X, y = X @ whitening.astype(LD).T, whitening.astype(LD) @ y
    n, d = X.shape
    mean, S = moments_ld(X)
    if shrinkage:
        s = np.sqrt(np.diag(S) + LD('1e-5'))
        S = ((1 - LD(penalty)) * (S / np.outer(s, s)) + LD(penalty) * np.eye(d, dtype=LD)) * np.outer(s, s)
    v = y - mean
    logdet, quad = chol_ld(S, v)
    if variant == 'standard':
        return -(d * np.log(2 * PI) + logdet + quad) / 2
    mpmath.mp.prec = 100          # the sum over x of _logc(d, n - 2) - _logc(d, n - 1) telescopes to two terms
    logc = LD(d) / 2 * np.log(LD(2)) + LD(str(mpmath.loggamma(mpmath.mpf(n - 1) / 2) - mpmath.loggamma(mpmath.mpf(n - 1 - d) / 2)))
    psi = chol_ld((n - 1) * S - np.outer(v, v) / (1 - LD(1) / n), v)
    if psi is None:
        return -LD(np.inf)
    logdet_psi = psi[0]
    return (-LD(d) / 2 * np.log(2 * PI) + logc - LD(d) / 2 * np.log(1 - LD(1) / n)
            - LD(n - d - 2) / 2 * (np.log(LD(n - 1)) + logdet) + LD(n - d - 3) / 2 * logdet_psi)


@pytest.fixture(scope='module')
def table():
    """case index -> (X, {config: (y, keywords, truth, |float64 reference - truth|)})"""
    out = {}
    for ci, case in enumerate(CASES):
        X, y, W, _ = R.make_case(*case)
        rows = {}
        for name in configs_of(case[1], case[2]):
            kw = dict(whitening=W) if CONFIGS[name] == 'W' else CONFIGS[name]
            yc = X.mean(0) + 0.2 * (y - X.mean(0)) if name == 'unbiased-near' else y
            t, ref = truth(X, yc, **kw), R.syn_loglik_ref(X, yc, **kw)[0, 0, 0]
            rows[name] = (yc, kw, t, abs(LD(ref) - t) if np.isfinite(t) else LD(0) if ref == t else LD(np.inf))
        out[ci] = (X, rows)
    return out


@pytest.mark.parametrize('ci', range(len(CASES)))
def test_parity_with_the_long_double_truth(table, ci):
    """Measured on an MI355X, the largest |device - truth| (bound) per case: 8.6e-12 (5.3e-11) at (80, 65), 1.4e-11
    (1.3e-10) at (96, 80), 4.9e-11 (1.4e-10) at (170, 145), 5.7e-13 (1.4e-10) at (40, 145), 1.0e-10 (2.2e-9) at (300, 256)."""
    import elfi_amd
    _, n, m = CASES[ci][:3]
    e_ref = max(float(row[3]) for cj in table if CASES[cj][2] == m for row in table[cj][1].values())
    assert np.isfinite(e_ref)
    X, rows = table[ci]
    worst = []
    for name, (y, kw, t, _) in rows.items():
        got = elfi_amd.wide_syn_loglik(X, y, **kw)
        if not np.isfinite(t):
            dev, bound = 0.0 if got == t else np.inf, 0.0
        else:
            dev, bound = float(abs(LD(got) - t)), max(16 * e_ref, 16 * np.spacing(abs(float(t))))
        print('n=%d m=%d %-9s loglik %.6e |device - truth| %.2e bound %.2e' % (n, m, name, got, dev, bound))
        worst.append((dev <= bound, name, dev, bound))
    assert all(w[0] for w in worst), [w[1:] for w in worst if not w[0]]


@pytest.mark.parametrize('m', [65, 145, 256])
def test_prefixes_penalties_groups_and_chunks_do_not_change_a_bit(hip_ctx, m):
    import elfi_amd
    n, G = 2 * m + 6, 3
    pre = sorted({m + 3, n // 2 + 1, n // 2 + 2, n - 1, n})      # boundaries inside a 4-row step
    pens = [0, 0.1, 0.45, 1]
    Xs = np.stack([R.make_case(30 + g, n, m, 0.7, 6.0)[0] for g in range(G)])
    y = R.make_case(30, n, m, 0.7, 6.0)[1]
    ll = elfi_amd.wide_syn_loglik(Xs, y, shrinkage='warton', prefixes=pre, penalties=pens)
    assert ll.shape == (G, len(pre), len(pens)) and np.all(np.isfinite(ll))
    for g in range(G):
        for k, p in enumerate(pre):
            for j, pen in enumerate(pens):
                assert ll[g, k, j] == elfi_amd.wide_syn_loglik(Xs[g, :p], y, shrinkage='warton', penalty=pen), (g, p, pen)
    hip_ctx.call('elfihip_syn_wide_set_cap', 1 << 20)       # one group and one slab per launch
    try:
        cut = elfi_amd.wide_syn_loglik(Xs, y, shrinkage='warton', prefixes=pre, penalties=pens)
    finally:
        hip_ctx.call('elfihip_syn_wide_set_cap', 0)
    assert np.array_equal(cut, ll)


def test_edges():
    import elfi_amd
    X, y, W, _ = R.make_case(*CASES[0])
    flat = X.copy()
    flat[:, 7] = 3.25                  # its shifted sums are exactly 0, so the pivot is exactly 0
    assert elfi_amd.wide_syn_loglik(flat, y) == -np.inf
    ll, mean, cov = elfi_amd.wide_syn_loglik(X, y, return_moments=True)
    mean_ld, cov_ld = moments_ld(X)
    assert np.array_equal(cov[0], cov[0].T)
    np.testing.assert_allclose(mean[0], mean_ld.astype(float), rtol=1e-13)
    np.testing.assert_allclose(cov[0], cov_ld.astype(float), rtol=1e-11, atol=1e-11)
    near = X.mean(0) + 0.2 * (y - X.mean(0))
    for lik in (elfi_amd.wide_standard_likelihood(shrinkage='warton', penalty=0.3), elfi_amd.wide_unbiased_likelihood()):
        out = lik(X, near[None, :])
        assert isinstance(out, np.ndarray) and out.shape == (1,) and np.isfinite(out[0])


WIDE = 'wide synthetic likelihood: %d summaries; 65 to 256 are supported (elfihip_syn_loglik takes 1 to 64)'
REJECTED = [
    (dict(m=64, ldx=64), WIDE % 64),
    (dict(m=257, ldx=257), WIDE % 257),
    (dict(variant=2), 'wide synthetic likelihood: variant 2; 0 (standard) and 1 (unbiased) are supported above 64 summaries'),
    (dict(n=1), 'bad shape G=1 n=1 m=65 ldx=65'),
    (dict(ldx=64), 'bad shape G=1 n=4 m=65 ldx=64'),
    (dict(variant=1, penalties=[0.5], P=1), 'penalties go with the standard variant only (variant 1)'),
]


@pytest.mark.parametrize('kw, text', REJECTED, ids=[str(i) for i in range(len(REJECTED))])
def test_invalid_call_is_an_argument_error_with_its_text(hip_ctx, kw, text):
    """Every call fails its checks before a pointer is read, so host arrays stand in for the _dev form's device pointers."""
    X, y, out = np.zeros((4, 257)), np.zeros(257), np.zeros(8)
    a = dict(n=4, m=65, ldx=65, variant=0, penalties=None, P=0)
    a.update(kw)
    pen = None if a['penalties'] is None else np.array(a['penalties'], dtype=np.float64)
    args = [X.ctypes.data, 1, a['n'], a['m'], a['ldx'], y.ctypes.data, None, a['variant'], None, 0,
            None if pen is None else pen.ctypes.data, a['P'], out.ctypes.data, None, None]
    for name in ('elfihip_syn_loglik_wide', 'elfihip_syn_loglik_wide_dev'):
        assert getattr(hip_ctx.lib, name)(hip_ctx.handle, *args) == ERR_ARG, name
        assert hip_ctx.lib.elfihip_last_error(hip_ctx.handle).decode() == text, name
    assert not out.any()
