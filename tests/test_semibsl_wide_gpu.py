"""GPU: the wide semiparametric synthetic likelihood (csrc/semibsl_wide.hip, 65 to 256 summaries) against a high-precision
truth computed here, bit for bit against itself over prefixes, penalties, groups and the chunking of its launches, its
edges and the rejections of its two C entry points.

Truth: Phi, Phi^-1, exp and log by mpmath at 100 bits on the float inputs, ranks by counting, scores at the exact rational
rank / (n + 1); the Gram matrix, the shrinkage, a column Cholesky factorisation and the forward solve in long double.
Bound of the parity test, the rule of tests/test_synlik.py (bound_for): 16 x the largest |float64 reference - truth| over
this file's cases and configurations of the same m (the reference is semibsl_ref.semi_loglik_ref), floored at 16 ulp of
|truth|.
"""
import functools

import mpmath
import numpy as np
import pytest

import semibsl_ref as R
import synlik_ref
from elfi_amd._lib import ERR_ARG
from test_synlik_wide_gpu import LD, chol_ld

pytestmark = pytest.mark.gpu

# (seed, n, m, rho, smax, tied): one column into the second 64-block, no multiple of 16, the scratch-assay width, n < m (the
# rank correlation is singular: the Warton configurations only), the maximum, and the scratch-assay shape with rows and y
# rounded to integers
CASES = [(41, 80, 65, 0.8, 5.0, False), (42, 96, 80, 0.6, 8.0, False), (43, 170, 145, 0.7, 10.0, False),
         (44, 40, 145, 0.7, 10.0, False), (45, 300, 256, 0.8, 5.0, False), (43, 170, 145, 0.7, 10.0, True)]
CONFIGS = {'none': {}, 'warton0.1': dict(shrinkage='warton', penalty=0.1), 'warton0.8': dict(shrinkage='warton', penalty=0.8)}


def make(case):
    X, y = synlik_ref.make_case(*case[:5])[:2]
    return (np.round(X), np.round(y)) if case[5] else (X, y)


def to_ld(x):
    return LD(mpmath.nstr(x, 30))


def truth_parts(X, y):
    """(sum of logpdf, eta (m), rho (m, m) unshrunk) of one group, in long double from 100-bit marginals."""
    mp = mpmath.mp
    mp.prec = 100
    n, m = X.shape
    ppf = lambda q: mp.sqrt(2) * mp.erfinv(2 * q - 1)
    score = {r2: to_ld(ppf(mp.mpf(r2) / (2 * (n + 1)))) for r2 in range(2, 2 * n + 1)}      # by twice the rank
    den = sum(score[2 * i] ** 2 for i in range(1, n + 1))
    Q = np.array([[score[int(2 * r)] for r in R.ranks(X[:, j])] for j in range(m)], dtype=LD).T
    eta, lps = np.zeros(m, dtype=LD), mp.mpf(0)
    for j in range(m):
        col = [mp.mpf(v) for v in X[:, j]]
        mean = mp.fsum(col) / n
        h = (mp.mpf(3) * n / 4) ** (-mp.mpf(1) / 5) * mp.sqrt(mp.fsum((c - mean) ** 2 for c in col) / (n - 1))
        z = [(mp.mpf(y[j]) - c) / h for c in col]
        lps += mp.log(mp.fsum(mp.exp(-v * v / 2) for v in z)) - mp.log(n) - mp.log(h) - mp.log(2 * mp.pi) / 2
        eta[j] = to_ld(ppf(min(mp.mpf(1), mp.fsum(mp.ncdf(v) for v in z) / n)))
    rho = Q.T @ Q / den
    np.fill_diagonal(rho, LD(1))
    return to_ld(lps), eta, rho


def truth(parts, penalty=None, **_):
    lps, eta, rho = parts
    if penalty is not None:
        rho = (1 - LD(penalty)) * rho + LD(penalty) * np.eye(len(eta), dtype=LD)
    logdet, quad = chol_ld(rho, eta)
    return -(logdet + (quad - eta @ eta)) / 2 + lps


@functools.lru_cache(maxsize=None)
def rows_of(ci):
    """(X, y, {config: (truth, |float64 reference - truth|)}) of CASES[ci]"""
    X, y = make(CASES[ci])
    parts = truth_parts(X, y)
    rows = {}
    for name, kw in CONFIGS.items():
        if kw or X.shape[0] > X.shape[1]:
            t = truth(parts, **kw)
            rows[name] = (t, abs(LD(R.semi_loglik_ref(X, y, **kw)[0, 0, 0]) - t))
    return X, y, rows


@pytest.mark.parametrize('ci', range(len(CASES)))
def test_parity_with_the_high_precision_truth(ci):
    """Measured on an MI355X, the largest |device - truth| (bound) per case: 7.5e-12 (2.5e-10) at (80, 65), 4.3e-13
    (5.8e-12) at (96, 80), 1.5e-12 (1.5e-10) at (170, 145), 2.9e-13 (1.5e-10) at (40, 145), 3.2e-11 (4.4e-10) at
    (300, 256), 2.7e-13 (1.5e-10) at the tied (170, 145)."""
    import elfi_amd
    n, m = CASES[ci][1:3]
    e_ref = max(float(row[1]) for cj in range(len(CASES)) if CASES[cj][2] == m for row in rows_of(cj)[2].values())
    assert np.isfinite(e_ref)
    X, y, rows = rows_of(ci)
    worst = []
    for name, (t, _) in rows.items():
        got = elfi_amd.wide_semi_loglik(X, y, **CONFIGS[name])
        dev, bound = float(abs(LD(got) - t)), max(16 * e_ref, 16 * np.spacing(abs(float(t))))
        print('n=%d m=%d %s%-9s loglik %.6e |device - truth| %.2e bound %.2e' % (n, m, 'tied ' if CASES[ci][5] else '', name, got, dev, bound))
        worst.append((dev <= bound, name, dev, bound))
    assert all(w[0] for w in worst), [w[1:] for w in worst if not w[0]]


@pytest.mark.parametrize('m', [65, 145, 256])
def test_prefixes_penalties_groups_and_chunks_do_not_change_a_bit(hip_ctx, m):
    import elfi_amd
    n, G = 2 * m + 6, 3
    pre = sorted({m + 3, n // 2 + 1, n // 2 + 2, n - 1, n})
    pens = [0, 0.1, 0.45, 1]
    Xs, y = synlik_ref.make_case(50, G * n, m, 0.7, 6.0)[:2]         # the groups share the columns' locations, so y is
    Xs = Xs.reshape(G, n, m)                                         # within reach of every group's density estimates
    ll = elfi_amd.wide_semi_loglik(Xs, y, shrinkage='warton', prefixes=pre, penalties=pens)
    assert ll.shape == (G, len(pre), len(pens)) and np.all(np.isfinite(ll[:, :, 1:]))
    for g in range(G):
        for k, p in enumerate(pre):
            for j, pen in enumerate(pens):
                assert ll[g, k, j] == elfi_amd.wide_semi_loglik(Xs[g, :p], y, shrinkage='warton', penalty=pen), (g, p, pen)
    hip_ctx.call('elfihip_syn_wide_set_cap', 1 << 20)       # one or two jobs per launch
    try:
        cut = elfi_amd.wide_semi_loglik(Xs, y, shrinkage='warton', prefixes=pre, penalties=pens)
    finally:
        hip_ctx.call('elfihip_syn_wide_set_cap', 0)
    assert np.array_equal(cut, ll)


def test_edges():
    import elfi_amd
    from elfi_amd import synlik
    X, y = make(CASES[0])
    n, m = X.shape
    flat = X.copy()
    flat[:, 7] = 3.25
    assert elfi_amd.wide_semi_loglik(flat, y) == -np.inf
    assert elfi_amd.wide_semi_loglik(X[:2], y) == -np.inf
    ll, u, rho, scores = elfi_amd.wide_semi_loglik(X, y, return_parts=True)
    assert u.shape == (1, m) and rho.shape == (1, m, m) and scores.shape == (1, n, m)
    _, u_ref, rho_ref, q_ref = R.parts(X, y)
    assert np.array_equal(rho[0], rho[0].T) and np.all(np.diag(rho[0]) == 1.0)
    print('u: max relative deviation %.2e; rho: %.2e' % (np.abs(u[0] / u_ref - 1).max(), np.abs(rho[0] / rho_ref - 1).max()))
    np.testing.assert_allclose(u[0], u_ref, rtol=1e-12)
    np.testing.assert_allclose(rho[0], rho_ref, rtol=1e-12)
    assert np.array_equal(np.argsort(scores[0], axis=0, kind='stable'), np.argsort(q_ref, axis=0, kind='stable'))
    out = elfi_amd.wide_semiparametric_likelihood(shrinkage='warton', penalty=0.3)(X, y[None, :])
    assert isinstance(out, np.ndarray) and out.shape == (1,) and np.isfinite(out[0])
    assert synlik._likelihood_setup(elfi_amd.wide_semiparametric_likelihood(), shrinkage='warton', whitening=None) == (
        elfi_amd.wide_semi_loglik, dict(shrinkage='warton', penalty=None))


WIDE = 'wide semiparametric likelihood: %d summaries; 65 to 256 are supported (elfihip_semi_loglik takes 1 to 64)'
ROWS = 'wide semiparametric likelihood: %d rows per group; 2 to 16384 are supported'
REJECTED = [(dict(m=64, ldx=64), WIDE % 64), (dict(m=257, ldx=257), WIDE % 257), (dict(n=1), ROWS % 1),
            (dict(n=16385), ROWS % 16385), (dict(ldx=64), 'bad shape G=1 n=4 m=65 ldx=64')]


@pytest.mark.parametrize('kw, text', REJECTED, ids=[str(i) for i in range(len(REJECTED))])
def test_invalid_call_is_an_argument_error_with_its_text(hip_ctx, kw, text):
    """Every call fails its checks before a pointer is read, so host arrays stand in for the _dev form's device pointers."""
    X, y, out = np.zeros((4, 257)), np.zeros(257), np.zeros(8)
    a = dict(n=4, m=65, ldx=65)
    a.update(kw)
    args = [X.ctypes.data, 1, a['n'], a['m'], a['ldx'], y.ctypes.data, None, 0, None, 0, out.ctypes.data, None, None, None]
    for name in ('elfihip_semi_loglik_wide', 'elfihip_semi_loglik_wide_dev'):
        assert getattr(hip_ctx.lib, name)(hip_ctx.handle, *args) == ERR_ARG, name
        assert hip_ctx.lib.elfihip_last_error(hip_ctx.handle).decode() == text, name
    assert not out.any()
