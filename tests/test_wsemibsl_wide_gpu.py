"""GPU: the wide whitened semiparametric synthetic likelihood (csrc/wsemibsl_wide.hip, 65 to 256 summaries) against a
high-precision truth computed here, bit for bit against itself over prefixes, penalties, groups and the chunking of its
launches, its edges and stages, the device-pointer form and the rejections of its two C entry points.

Truth: the marginals and the scores of tests/test_semibsl_wide_gpu.py (mpmath at 100 bits); T = Q W^T, the ranks of its
columns by counting, rho, C = cov(Q), d, eta_w, the scaled matrix, a column Cholesky factorisation and the forward solve in
long double.  Bound of the parity test, the rule of tests/test_synlik.py (bound_for): 16 x the largest |float64 reference -
truth| over this file's cases and configurations of the same m (the reference is wsemibsl_ref.wsemi_loglik_ref), floored at
16 ulp of |truth|.  Precondition, asserted on the reference's T: no gap within a column of T is below wsemibsl_ref.MIN_GAP,
so rounding changes no rank (7.0e-6, 8.7e-8, 3.9e-5, 3.1e-7 and 1.8e-6 for the five cases), and every d lies in 0.65 to 1.91.
"""
import functools

import mpmath
import numpy as np
import pytest

import device_layout as DL
import synlik_ref
import wsemibsl_ref as R
from elfi_amd._lib import ERR_ARG
from test_semibsl_wide_gpu import to_ld, truth_parts
from test_synlik_wide_gpu import LD, chol_ld

pytestmark = pytest.mark.gpu

# (seed, n, m, rho, smax, tied): one column into the second 64-block, the scratch-assay width, n < m (the rank correlation
# is singular: the Warton configurations only), the maximum, and the scratch-assay shape with rows and y rounded to integers
CASES = [(41, 80, 65, 0.8, 5.0, False), (43, 170, 145, 0.7, 10.0, False), (44, 40, 145, 0.7, 10.0, False),
         (45, 300, 256, 0.8, 5.0, False), (43, 170, 145, 0.7, 10.0, True)]
CONFIGS = {'none': {}, 'warton0.1': dict(shrinkage='warton', penalty=0.1), 'warton0.8': dict(shrinkage='warton', penalty=0.8)}


@functools.lru_cache(maxsize=None)
def make(ci):
    """(X, y, W) of CASES[ci]; W by the recipe of wsemibsl_ref.whitening_matrix."""
    seed, n, m, corr, scale, tied = CASES[ci]
    X, y = synlik_ref.make_case(seed, n, m, corr, scale)[:2]
    if tied:
        X, y = np.round(X), np.round(y)
    D = synlik_ref.make_case(seed + 1000, 4 * m + 50, m, corr, scale)[0]
    Q = R.S.parts(D, D[0])[3]
    w, v = np.linalg.eigh(np.cov((Q - Q.mean(0)) / Q.std(0), rowvar=False))
    return X, y, np.round(np.diag(w ** -0.5) @ v.T, 8)


def truth_wparts(X, y, W):
    """(sum of logpdf, eta_w (m), rho (m, m) unshrunk, d (m)) of one group, in long double from 100-bit marginals."""
    lps, eta, _ = truth_parts(X, y)
    mp = mpmath.mp
    mp.prec = 100
    n, m = X.shape
    ppf = lambda q: mp.sqrt(2) * mp.erfinv(2 * q - 1)
    score = {r2: to_ld(ppf(mp.mpf(r2) / (2 * (n + 1)))) for r2 in range(2, 2 * n + 1)}      # by twice the rank
    den = sum(score[2 * i] ** 2 for i in range(1, n + 1))
    scores_of = lambda A: np.array([[score[int(2 * r)] for r in R.S.ranks(A[:, j])] for j in range(m)], dtype=LD).T
    Wl = W.astype(LD)
    Q = scores_of(X)
    Q2 = scores_of(Q @ Wl.T)
    rho = Q2.T @ Q2 / den
    np.fill_diagonal(rho, LD(1))
    D = Q - Q.sum(0) / n
    d = np.sqrt(np.diag(Wl @ (D.T @ D / (n - 1)) @ Wl.T))
    return lps, Wl @ eta, rho, d


def truth(parts, penalty=None, **_):
    lps, ew, rho, d = parts
    if penalty is not None:
        rho = (1 - LD(penalty)) * rho + LD(penalty) * np.eye(len(d), dtype=LD)
    logdet, quad = chol_ld(d[:, None] * rho * d[None, :], ew)
    return -(logdet + (quad - ew @ ew)) / 2 + lps


@functools.lru_cache(maxsize=None)
def rows_of(ci):
    """{config: (truth, |float64 reference - truth|)} of CASES[ci], after the precondition on the reference's T and d."""
    X, y, W = make(ci)
    _, _, _, d, _, T = R.wparts(X, y, W)
    assert np.diff(np.sort(T, axis=0), axis=0).min() >= R.MIN_GAP
    assert 0.65 <= d.min() and d.max() <= 1.91
    parts = truth_wparts(X, y, W)
    rows = {}
    for name, kw in CONFIGS.items():
        if kw or X.shape[0] > X.shape[1]:
            t = truth(parts, **kw)
            rows[name] = (t, abs(LD(R.wsemi_loglik_ref(X, y, W, **kw)) - t))
    return rows


@pytest.mark.parametrize('ci', range(len(CASES)))
def test_parity_with_the_high_precision_truth(ci):
    """Measured on an MI355X, the largest |device - truth| (bound) per case: 2.2e-12 (3.4e-11) at (80, 65), 1.6e-13
    (5.5e-11) at (170, 145), 9.3e-13 (5.5e-11) at (40, 145), 5.0e-12 (6.9e-12) at (300, 256), 2.1e-13 (5.5e-11) at the tied
    (170, 145).  At 256 the float64 reference happens to land within 4.3e-13 of the truth, so that bound is the tightest."""
    import elfi_amd
    n, m = CASES[ci][1:3]
    e_ref = max(float(row[1]) for cj in range(len(CASES)) if CASES[cj][2] == m for row in rows_of(cj).values())
    assert np.isfinite(e_ref)
    X, y, W = make(ci)
    worst = []
    for name, (t, _) in rows_of(ci).items():
        got = elfi_amd.wide_wsemi_loglik(X, y, W, **CONFIGS[name])
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
    W = make([c[2] for c in CASES].index(m))[2]
    ll = elfi_amd.wide_wsemi_loglik(Xs, y, W, shrinkage='warton', prefixes=pre, penalties=pens)
    assert ll.shape == (G, len(pre), len(pens)) and np.all(np.isfinite(ll[:, :, 1:]))
    for g in range(G):
        for k, p in enumerate(pre):
            for j, pen in enumerate(pens):
                assert ll[g, k, j] == elfi_amd.wide_wsemi_loglik(Xs[g, :p], y, W, shrinkage='warton', penalty=pen), (g, p, pen)
    hip_ctx.call('elfihip_syn_wide_set_cap', 1 << 20)       # one job per launch
    try:
        cut = elfi_amd.wide_wsemi_loglik(Xs, y, W, shrinkage='warton', prefixes=pre, penalties=pens)
    finally:
        hip_ctx.call('elfihip_syn_wide_set_cap', 0)
    assert np.array_equal(cut, ll)


def test_edges_and_stages():
    import elfi_amd
    from elfi_amd import synlik
    X, y, W = make(0)
    n, m = X.shape
    flat = X.copy()
    flat[:, 7] = 3.25
    assert elfi_amd.wide_wsemi_loglik(flat, y, W) == -np.inf
    assert elfi_amd.wide_wsemi_loglik(X[:2], y, W) == -np.inf
    ll, u, rho, scale, scores = elfi_amd.wide_wsemi_loglik(X, y, W, return_parts=True)
    assert u.shape == (1, m) and rho.shape == (1, m, m) and scale.shape == (1, m) and scores.shape == (1, n, m)
    _, _, rho_ref, d_ref, _, T = R.wparts(X, y, W)
    assert np.array_equal(rho[0], rho[0].T) and np.all(np.diag(rho[0]) == 1.0)
    print('rho: max relative deviation %.2e; scale: %.2e' % (np.abs(rho[0] / rho_ref - 1).max(), np.abs(scale[0] / d_ref - 1).max()))
    np.testing.assert_allclose(rho[0], rho_ref, rtol=1e-12)
    np.testing.assert_allclose(scale[0], d_ref, rtol=1e-12)
    assert np.array_equal(np.argsort(scores[0], axis=0, kind='stable'), np.argsort(T, axis=0, kind='stable'))
    lik = elfi_amd.wide_whitened_semiparametric_likelihood(W, shrinkage='warton', penalty=0.3)
    out = lik(X, y[None, :])
    assert isinstance(out, np.ndarray) and out.shape == (1,) and np.isfinite(out[0])
    batched, setup = synlik._likelihood_setup(lik, shrinkage='warton', whitening=None)
    assert batched is elfi_amd.wide_wsemi_loglik and setup['whitening'] is W and setup['penalty'] == 0.3


def test_device_pointer_form_at_a_pitch_and_an_offset_equals_the_host_form(hip_ctx):
    import elfi_amd
    import torch
    from elfi_amd import _lib
    X, y, W = make(0)
    m = X.shape[1]
    G, ng, ldx = 1, len(X), m + 3
    pre, pens = np.array([ng // 2 + 1, ng], dtype=np.int64), np.array([0.1, 0.6])
    want, wu, wrho, wd, wsc = elfi_amd.wide_wsemi_loglik(X[None], y, W, prefixes=pre, shrinkage='warton',
                                                         penalties=list(pens), return_parts=True)
    assert want.shape == (G, 2, 2) and np.all(np.isfinite(want))
    (keep, dX), (keep_y, dy), (keep_w, dW) = DL.place(X, ldx, 1), DL.place(y[None, :], m, 1), DL.place(W, m, 1)
    oll, ou, od = DL.guarded_out(G, 4, off=1), DL.guarded_out(G, m), DL.guarded_out(G, m, off=1)
    orho, osc = DL.guarded_out(G, m * m, off=1), DL.guarded_out(G * ng, m)
    torch.cuda.synchronize()
    hip_ctx.call("elfihip_wsemi_loglik_wide_dev", dX, G, ng, m, ldx, dy, dW, _lib.ptr(pre), len(pre), _lib.ptr(pens),
                 len(pens), oll.ptr, ou.ptr, orho.ptr, od.ptr, osc.ptr)
    hip_ctx.synchronize()
    assert np.array_equal(oll.check().reshape(want.shape), want)
    assert np.array_equal(ou.check(), wu) and np.array_equal(orho.check().reshape(wrho.shape), wrho)
    assert np.array_equal(od.check(), wd) and np.array_equal(osc.check().reshape(wsc.shape), wsc)


WIDE = 'wide whitened semiparametric likelihood: %d summaries; 65 to 256 are supported (elfihip_wsemi_loglik takes 1 to 64)'
ROWS = 'wide whitened semiparametric likelihood: %d rows per group; 2 to 16384 are supported'
REJECTED = [(dict(m=64, ldx=64), WIDE % 64), (dict(m=257, ldx=257), WIDE % 257), (dict(n=1), ROWS % 1),
            (dict(n=16385), ROWS % 16385), (dict(ldx=64), 'bad shape G=1 n=4 m=65 ldx=64'),
            (dict(W=None), 'the whitening matrix is NULL')]


@pytest.mark.parametrize('kw, text', REJECTED, ids=[str(i) for i in range(len(REJECTED))])
def test_invalid_call_is_an_argument_error_with_its_text(hip_ctx, kw, text):
    """Every call fails its checks before a pointer is read, so host arrays stand in for the _dev form's device pointers."""
    X, y, W, out = np.zeros((4, 257)), np.zeros(257), np.zeros((257, 257)), np.zeros(8)
    a = dict(n=4, m=65, ldx=65, W=W.ctypes.data)
    a.update(kw)
    args = [X.ctypes.data, 1, a['n'], a['m'], a['ldx'], y.ctypes.data, a['W'], None, 0, None, 0, out.ctypes.data, None, None,
            None, None]
    for name in ('elfihip_wsemi_loglik_wide', 'elfihip_wsemi_loglik_wide_dev'):
        assert getattr(hip_ctx.lib, name)(hip_ctx.handle, *args) == ERR_ARG, name
        assert hip_ctx.lib.elfihip_last_error(hip_ctx.handle).decode() == text, name
    assert not out.any()
