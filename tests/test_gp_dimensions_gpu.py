"""The GP at every input dimension elfihip_gp_create accepts (1 <= d <= 256): a sweep over both sides of every width at
which the device code takes another path, through GPHandle against oracle/gp_oracle.py's Posterior.

The padded width dp = round_up(d, 4) decides (csrc/gp_predict.hip, gp_fit.hip, gp_hyper.hip, gp_dense.hip):
  dp <= 16 / > 16     grad_rows: one round of sixteen dimensions, or several
  dp <= 24 / > 24     query points and a one-point append travel in kernel arguments, or are uploaded; calls with many
                      points take the dense form, or stay on the streaming form (S = 130: nine passes in two groups)
  dp <= 44 / >= 48    kinv_grad_kernel stages X in LDS, or reads it from global memory
  dp <= 64 / > 64     finish_kernel stores gradients from wave 0 only, or from several waves; gram_kernel stages X in
                      one chunk of columns, or in several
  dp <= 156 / >= 160  gram_kernel before this sweep asked for 1024 (dp + 1) bytes of LDS: 164 864 at dp = 160, more than
                      the 160 KiB of a CU, so no d >= 157 could be factorised.  It now stages 64 columns at a time.
  d = 256 / 257       accepted / refused
DIMS holds both sides of each.

Inputs.  tests/test_gp_gpu.py's _problem (X uniform in [-2, 2]^d) with G.default_hyper and the lengthscale multiplied by
sqrt(d / 2) (the default at d = 2): the squared distance between two points grows like d, so the unscaled default leaves
no correlation between any two points from d = 30 or so on (largest off-diagonal k / var 4e-12 at d = 70) and a kernel
that dropped coordinates would go unnoticed.  With the scaling, at n = 200 and every d of DIMS the median off-diagonal
k / var is 0.22 to 0.23 and cond(K + noise I) 200 to 720 -- the regime of the d = 2 cases of test_gp_gpu.py (2e3), so
that file's tolerances, and test_gp_hyper_gpu.py's, are used unchanged:
  L 1e-10, L^-T 1e-9, alpha 1e-8, log Z 1e-9; mu 1e-8, var 1e-8 (var + bias), dmu 1e-8, dvar 1e-7 of the largest entry;
  gradient of log Z 1e-7 of the largest component; LCB 1e-8, LCB gradient 1e-7; the two lock-step forms against each
  other 1e-9 / 1e-8 (test_lockstep_kinv_gpu.py); extend against rebuild as test_extend_matches_rebuild.

Sensitivity (test_every_coordinate_matters, on the oracle alone, no GPU): with column d - 1 of X and of the query points
set to zero -- what an implementation that ignored only the last real coordinate would compute -- every compared quantity
moves by at least 1000 times its tolerance.  Measured ratios of change to tolerance (n = 200, S = 17, beta = 3):
    d        L     L^-T    alpha       mu      var      dmu     dvar  grad logZ    lcb  lcb grad
   16  2.1e+09  2.7e+08  5.4e+07  5.4e+06  4.7e+06  7.7e+07  6.5e+06  1.0e+06  1.2e+07  6.3e+06
   17  1.3e+09  1.6e+08  1.7e+07  3.2e+06  4.1e+06  6.7e+07  5.3e+06  9.1e+05  7.0e+06  7.0e+06
   24  7.8e+08  1.1e+08  1.6e+07  2.5e+06  5.3e+06  4.6e+07  9.4e+06  4.3e+05  6.8e+06  5.7e+06
   25  9.6e+08  1.1e+08  1.9e+07  2.7e+06  6.0e+06  5.6e+07  9.7e+06  3.7e+05  1.0e+07  7.2e+06
   44  4.1e+08  4.3e+07  1.4e+07  2.2e+06  4.0e+06  5.7e+07  9.4e+06  1.5e+05  5.1e+06  8.5e+06
   45  5.4e+08  5.8e+07  5.7e+06  1.2e+06  3.0e+06  4.4e+07  8.5e+06  1.9e+05  3.7e+06  7.4e+06
   64  2.6e+08  3.1e+07  1.1e+07  1.1e+06  1.7e+06  5.8e+07  7.4e+06  1.2e+05  1.2e+06  5.8e+06
   65  2.8e+08  4.5e+07  1.0e+07  1.4e+06  2.3e+06  7.4e+07  8.9e+06  1.3e+05  3.4e+06  8.6e+06
  156  9.2e+07  1.2e+07  4.6e+06  2.5e+05  5.2e+05  4.9e+07  6.5e+06  6.4e+04  5.7e+05  5.8e+06
  157  9.0e+07  1.2e+07  7.2e+06  4.8e+05  5.5e+05  7.0e+07  6.8e+06  5.4e+04  9.2e+05  7.2e+06
  256  5.3e+07  6.4e+06  2.8e+06  3.3e+05  4.5e+05  7.4e+07  8.2e+06  3.0e+04  6.6e+05  8.3e+06
(the smallest is 3.0e4, gradient of log Z at d = 256: thirty times the 1000 the guard asks for; the gradients' own last
column goes to zero with the coordinate, which is why dmu moves most)

Largest error observed on an MI355X per d, as a fraction of its tolerance (1.0 = at the tolerance), over all the cases
of this file that compare the quantity with the oracle:
    d        L     L^-T    alpha     logZ       mu      var      dmu     dvar  grad logZ    lcb  lcb grad  forms 3/2  extend/rebuild
   16  3.0e-05  6.1e-06  1.9e-06  0.0e+00  1.9e-07  1.7e-06  6.6e-07  9.3e-07  4.6e-09  2.4e-06  7.4e-07  1.4e-05        -
   17  2.3e-05  3.5e-06  1.3e-06  0.0e+00  2.9e-07  9.2e-07  6.6e-07  9.9e-07  6.0e-09  2.0e-06  1.3e-06  8.0e-06        -
   24  2.2e-05  3.2e-06  7.4e-07  1.6e-07  1.2e-07  7.6e-07  8.9e-07  6.9e-07  4.2e-09  7.8e-07  3.0e-07  4.2e-06  8.4e-06
   25  2.0e-05  3.9e-06  5.6e-07  1.6e-07  1.3e-07  8.6e-07  9.7e-07  4.3e-07  6.4e-09  1.4e-06  3.1e-07  1.1e-05  6.8e-06
   44  1.6e-05  2.4e-06  1.2e-06  1.4e-07  1.2e-07  5.8e-07  5.6e-07  4.6e-07  3.2e-09  2.0e-07  1.1e-07  2.6e-06        -
   45  1.1e-05  2.0e-06  9.7e-07  0.0e+00  1.1e-07  6.6e-07  6.5e-07  6.9e-07  8.1e-10  5.7e-07  2.0e-07  4.2e-06        -
   64  1.2e-05  1.7e-06  1.3e-06  0.0e+00  1.4e-07  4.5e-07  5.0e-07  3.9e-07  1.1e-09  4.5e-07  1.1e-07  3.0e-06        -
   65  1.2e-05  2.0e-06  1.1e-06  1.3e-07  1.2e-07  7.0e-07  5.4e-07  8.0e-07  2.1e-09  8.5e-07  2.0e-07  3.0e-06  5.0e-06
  156  1.1e-05  1.4e-06  9.8e-07  0.0e+00  8.9e-08  5.1e-07  3.5e-07  6.9e-07  3.7e-09  6.1e-07  1.2e-07  5.2e-06        -
  157  1.1e-05  1.4e-06  1.0e-06  0.0e+00  1.1e-07  4.9e-07  4.0e-07  9.8e-07  1.9e-09  5.7e-07  1.0e-07  2.0e-06        -
  256  9.3e-06  1.1e-06  1.3e-06  1.2e-07  1.1e-07  4.1e-07  4.7e-07  6.0e-07  2.6e-09  6.8e-07  1.0e-07  6.8e-06  4.2e-06
(0.0: the two log Z agree to the last bit; d = 65 also: bordered K^-1 1.8e-07 of its 1e-8; MaxVar value 1.1e-07 / 4.0e-08
of its 1e-7 at d = 25 / 65.  Every figure is five orders or more inside its tolerance and at least nine orders below what
dropping one coordinate does; each test prints its figures -- lines starting with DIMERR under pytest -s -- before it
holds them to the tolerance.)
No tolerance differs from the existing ones.
"""
import numpy as np
import pytest

import gp_oracle as G
from test_gp_gpu import _problem

DIMS = (16, 17, 24, 25, 44, 45, 64, 65, 156, 157, 256)
N = 200
BETA = 3.0

gpu = pytest.mark.gpu


# ---- inputs ------------------------------------------------------------------------------------------------------------
def scaled_hyper(bounds, y, d):
    h = dict(G.default_hyper(bounds, y))
    h['ls'] *= np.sqrt(d / 2.0)
    return h


_CASES = {}


def _case(d, n=N):
    """(X, y, bounds, hyper, CPU posterior) of the sweep's problem at (n, d); computed once, never modified."""
    if (n, d) not in _CASES:
        X, y, bounds = _problem(n, d, seed=n + d)
        h = scaled_hyper(bounds, y, d)
        _CASES[(n, d)] = (X, y, bounds, h, G.Posterior(X, y, h['var'], h['ls'], h['bias'], h['noise']))
    return _CASES[(n, d)]


def _queries(X, S, seed=3):
    xs = np.random.RandomState(seed + S).uniform(-2, 2, (S, X.shape[1]))
    xs[0] = X[0]                      # exactly on an evidence point
    if S > 2:
        xs[1] = X[1] + 1e-4           # and next to one: the smallest variances
    return xs


def _lcb(post, xs, beta):
    """mu - sqrt(beta var) and its gradient from the oracle's prediction (G.lcb_beta overflows for large d)."""
    mu, var = post.predict(xs, noiseless=True)
    gmu, gvar = post.predictive_gradients(xs)
    return mu - np.sqrt(beta * var), gmu - 0.5 * gvar * np.sqrt(beta / var)


def _device(X, y, h, capacity=None):
    from elfi_amd.gp import GPHandle
    gp = GPHandle(X.shape[1], capacity or X.shape[0])
    gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    gp.set_data(X, y)
    return gp, gp.factorize()


# ---- comparisons: every figure is printed before it is held to its tolerance ---------------------------------------------
def _scaled(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / (np.max(np.abs(b)) + 1e-300)


def _hold(d, what, err, tol):
    print('DIMERR d=%d %s err=%.3e tol=%.0e frac=%.3g' % (d, what, err, tol, err / tol))
    assert err <= tol, '%s at d = %d: %g > %g' % (what, d, err, tol)


def _hold_factor(d, gp, logz, post, tag=''):
    _hold(d, 'L' + tag, _scaled(gp.get(0), post.L), 1e-10)
    _hold(d, 'L^-T' + tag, _scaled(gp.get(1), post.Linv.T), 1e-9)
    _hold(d, 'alpha' + tag, _scaled(gp.get(2), post.alpha), 1e-8)
    _hold(d, 'logZ' + tag, abs(logz - post.log_marginal) / abs(post.log_marginal), 1e-9)


def _hold_prediction(d, post, xs, mu, var, dmu=None, dvar=None, tag=''):
    rmu, rvar = post.predict(xs, noiseless=True)
    _hold(d, 'mu' + tag, _scaled(mu, rmu), 1e-8)
    _hold(d, 'var' + tag, np.max(np.abs(var - rvar)) / (post.var + post.bias), 1e-8)
    if dmu is not None:
        gmu, gvar = post.predictive_gradients(xs)
        _hold(d, 'dmu' + tag, _scaled(dmu, gmu), 1e-8)
        _hold(d, 'dvar' + tag, _scaled(dvar, gvar), 1e-7)


# ---- the guard: the sweep's inputs make every coordinate count (CPU, oracle only) ----------------------------------------
def _quantities(X, y, h, xs):
    p = G.Posterior(X, y, h['var'], h['ls'], h['bias'], h['noise'])
    mu, var = p.predict(xs, noiseless=True)
    dmu, dvar = p.predictive_gradients(xs)
    val, grad = _lcb(p, xs, BETA)
    return dict(L=p.L, LinvT=p.Linv.T, alpha=p.alpha, mu=mu, var=var, dmu=dmu, dvar=dvar, glogZ=p.log_marginal_grad(),
                lcb=val, lcb_grad=grad), p


SENSITIVITY_TOL = dict(L=1e-10, LinvT=1e-9, alpha=1e-8, mu=1e-8, var=1e-8, dmu=1e-8, dvar=1e-7, glogZ=1e-7, lcb=1e-8,
                       lcb_grad=1e-7)


def sensitivity_ratios(d, n=N, S=17):
    """Change of every compared quantity when coordinate d - 1 is ignored, in units of the quantity's tolerance."""
    X, y, bounds, h, _ = _case(d, n)
    xs = _queries(X, S)
    full, p = _quantities(X, y, h, xs)
    X0, xs0 = X.copy(), xs.copy()
    X0[:, d - 1] = 0.0
    xs0[:, d - 1] = 0.0
    cut, _ = _quantities(X0, y, h, xs0)
    out = {}
    for k, tol in SENSITIVITY_TOL.items():
        change = (np.max(np.abs(cut[k] - full[k])) / (p.var + p.bias) if k == 'var' else _scaled(cut[k], full[k]))
        out[k] = change / tol
    return out


@pytest.mark.parametrize('d', DIMS)
def test_every_coordinate_matters(d):
    X, y, bounds, h, post = _case(d)
    r2 = G.rbf_r2(X)
    k = np.exp(-0.5 * r2[np.triu_indices(N, 1)] / h['ls'] ** 2)
    Ky = post.K + (h['noise'] + G.JITTER) * np.eye(N)
    print('d=%d median k/var %.3g largest %.3g cond %.3g' % (d, np.median(k), k.max(), np.linalg.cond(Ky)))
    assert 0.1 <= np.median(k) <= 0.5, 'the evidence points must stay correlated'
    assert np.linalg.cond(Ky) <= 2e3, 'the conditioning of the d = 2 cases whose tolerances are used'
    ratios = sensitivity_ratios(d)
    print('SENS d=%d ' % d + ' '.join('%s=%.2g' % kv for kv in ratios.items()))
    for name, r in ratios.items():
        assert r >= 1000, '%s at d = %d: ignoring coordinate d - 1 moves it by only %g tolerances' % (name, d, r)


# ---- factorisation ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('d', DIMS)
def test_factorize(hip_ctx, d):
    X, y, bounds, h, post = _case(d)
    gp, logz = _device(X, y, h)
    _hold_factor(d, gp, logz, post)
    L, WT = gp.get(0), gp.get(1)
    assert np.allclose(L @ WT.T, np.eye(N), atol=1e-8)       # L lower, L^-T upper, L L^-1 = I
    assert np.array_equal(gp.get(3), X)
    if d in (65, 256):
        for schedule in (1, 2):
            gp.set_schedule(schedule)
            _hold_factor(d, gp, gp.factorize(), post, ' (schedule %d)' % schedule)
    gp.close()


# ---- prediction and gradients ----------------------------------------------------------------------------------------
# S = 1, 7: one pass (d <= 24: the points in the kernel arguments; above: read from pinned memory; with gradients the
# copy-free call whose results finish_kernel stores to the host, from several waves at d >= 65); S = 17: two passes;
# S = 130: the dense form at d <= 24, nine streaming passes in two groups above
@gpu
@pytest.mark.parametrize('S', [1, 7, 17, 130])
@pytest.mark.parametrize('d', DIMS)
def test_predict_and_gradients(hip_ctx, d, S):
    X, y, bounds, h, post = _case(d)
    gp, _ = _device(X, y, h)
    xs = _queries(X, S)
    mu, var = gp.predict(xs, noiseless=True)
    m3, v3, dmu, dvar = gp.predict_grad(xs)
    _hold_prediction(d, post, xs, mu, var, tag=' (S=%d)' % S)
    _hold_prediction(d, post, xs, m3, v3, dmu, dvar, tag=' (S=%d, with gradients)' % S)
    mu_n, var_n = gp.predict(xs, noiseless=False)
    assert np.array_equal(mu_n, mu) and np.allclose(var_n, var + post.noise, rtol=1e-14, atol=0)
    # the same call again: bit for bit
    mu2, var2 = gp.predict(xs, noiseless=True)
    again = gp.predict_grad(xs)
    assert np.array_equal(mu2, mu) and np.array_equal(var2, var)
    for a, b in zip(again, (m3, v3, dmu, dvar)):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(dmu)) and np.all(np.isfinite(dvar))
    gp.close()


# ---- LCB: the two lock-step forms ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('d', DIMS)
def test_lcb_in_both_lockstep_forms(hip_ctx, d):
    X, y, bounds, h, post = _case(d)
    gp, _ = _device(X, y, h)
    xs = _queries(X, 7)
    rval, rgrad = _lcb(post, xs, BETA)
    out = {}
    for form in (2, 3):
        gp.set_lockstep_form(form)
        val, grad = gp.lcb(xs, BETA)
        assert gp.lockstep_info()[0] == (form == 3), 'form %d: K^-1 in use %r' % (form, gp.lockstep_info())
        _hold(d, 'lcb (form %d)' % form, _scaled(val, rval), 1e-8)
        _hold(d, 'lcb gradient (form %d)' % form, _scaled(grad, rgrad), 1e-7)
        v2, g2 = gp.lcb(xs, BETA)
        assert np.array_equal(v2, val) and np.array_equal(g2, grad)
        vo, _ = gp.lcb(xs, BETA, with_grad=False)
        _hold(d, 'lcb value-only call (form %d)' % form, _scaled(vo, rval), 1e-8)
        out[form] = (val, grad)
    _hold(d, 'lcb, K^-1 product against the triangular products', _scaled(out[3][0], out[2][0]), 1e-9)
    _hold(d, 'lcb gradient, K^-1 product against the triangular products', _scaled(out[3][1], out[2][1]), 1e-8)
    gp.close()


@gpu
@pytest.mark.parametrize('d', [25, 65])
def test_lcb_minimize(hip_ctx, d):
    X, y, bounds, h, post = _case(d)
    gp, _ = _device(X, y, h)
    gp.set_lockstep_form(2)      # one form for the search and for the re-evaluation below
    starts = np.random.RandomState(d).uniform(-2, 2, (5, d))
    f0, _ = gp.lcb(starts, BETA)
    locs, vals, iters, n_eval = gp.lcb_minimize(starts, bounds, BETA)
    scale = np.max(np.abs(f0)) + 1.0
    lo, hi = np.array(bounds).T
    assert np.all(locs >= lo) and np.all(locs <= hi)
    again, _ = gp.lcb(locs, BETA)
    # two device evaluations of one point through the same kernels (1e-12: a row against the call with that row alone)
    assert np.max(np.abs(vals - again[:, 0])) <= 1e-12 * scale, np.max(np.abs(vals - again[:, 0]))
    assert np.all(vals <= f0[:, 0] + 1e-12 * scale), (vals, f0[:, 0])
    assert np.any(vals < f0[:, 0] - 1e-6 * scale), 'the search must move'
    _hold(d, 'lcb at the end points of the search', np.max(np.abs(vals - _lcb(post, locs, BETA)[0][:, 0])) / scale, 1e-8)
    assert n_eval >= 5 and np.all(iters <= 1000)
    gp.close()


# ---- gradient of the log marginal likelihood ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('d', DIMS)
def test_nlml_grad(hip_ctx, d):
    X, y, bounds, h, post = _case(d)
    gp, logz = _device(X, y, h)
    lz, g = gp.nlml_grad()
    assert lz == logz
    rg = post.log_marginal_grad()
    _hold(d, 'gradient of log Z', np.max(np.abs(g - rg)) / np.max(np.abs(rg)), 1e-7)
    if d == 65:
        # the lengthscale component is the derivative of what factorize() returns (test_gradient_with_other_hyperparameters)
        eps = 1e-5
        f = []
        for ls in (h['ls'] + eps, h['ls'] - eps):
            gp.set_hyper(h['var'], ls, h['bias'], h['noise'])
            f.append(gp.factorize())
        fd = (f[0] - f[1]) / (2 * eps)
        assert abs(fd - g[1]) <= 1e-5 * (1 + abs(g[1])), (fd, g[1])
    gp.close()


# ---- extend, append ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('n0,k', [(126, 4), (200, 3)])       # across 128 (the third point rebuilds), inside a block
@pytest.mark.parametrize('d', [24, 25, 65, 256])
def test_extend_and_append(hip_ctx, d, n0, k):
    from elfi_amd.gp import GPHandle
    n = n0 + k
    X, y, bounds, h, post = _case(d, n)
    a, _ = _device(X[:n0], y[:n0], h, capacity=n)
    kinv = d == 65 and n0 == 200
    if kinv:
        a.set_lockstep_form(3)
        a.lcb(_queries(X, 7), BETA)
        assert a.lockstep_info()[0]
    for i in range(n0, n):
        lz_a = a.extend(X[i:i + 1], y[i:i + 1])               # one point at a time: the bordering path
    b, lz_b = _device(X, y, h)
    assert abs(lz_a - lz_b) <= 1e-10 * abs(lz_b)
    _hold(d, 'logZ after extend', abs(lz_a - post.log_marginal) / abs(post.log_marginal), 1e-9)
    for which, tol in ((0, 1e-10), (1, 1e-9), (2, 1e-8)):
        _hold(d, 'extend against rebuild, item %d' % which, _scaled(a.get(which), b.get(which)), tol)
    _hold(d, 'L after extend', _scaled(a.get(0), post.L), 1e-10)
    assert np.array_equal(a.get(3), X) and np.array_equal(a.get(4), y)
    xs = _queries(X, 6)
    m, v, dmu, dvar = a.predict_grad(xs)
    _hold_prediction(d, post, xs, m, v, dmu, dvar, tag=' after extend')
    _, g = a.nlml_grad()
    rg = post.log_marginal_grad()
    _hold(d, 'gradient of log Z after extend', np.max(np.abs(g - rg)) / np.max(np.abs(g)), 1e-7)
    if kinv:
        assert a.lockstep_info()[0], 'an extend inside the padded size keeps K^-1'
        _hold(d, 'bordered K^-1', _scaled(a.get(5), post.Kinv), 1e-8)
        val, grad = a.lcb(xs, BETA)
        rval, rgrad = _lcb(post, xs, BETA)
        _hold(d, 'lcb after extend (K^-1 form)', _scaled(val, rval), 1e-8)
        _hold(d, 'lcb gradient after extend (K^-1 form)', _scaled(grad, rgrad), 1e-7)
    # one appended row + factorize == set_data of everything: the same evidence on the device, the same factor
    c = GPHandle(d, n)
    c.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    c.set_data(X[:n - 1], y[:n - 1])
    c.append(X[n - 1:], y[n - 1:])
    lz_c = c.factorize()
    assert np.array_equal(c.get(3), X) and np.array_equal(c.get(4), y)
    assert lz_c == lz_b and np.array_equal(c.get(0), b.get(0)) and np.array_equal(c.get(2), b.get(2))
    for gp in (a, b, c):
        gp.close()


# ---- prior kernel matrix, cross covariance, MaxVar -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('d', [25, 65])
def test_kernel_matrix(hip_ctx, d):
    """GPy's kern.K(X, X2) as in test_prior_kernel_matrix_is_gpys_kern_K, at the sweep's hyper-parameters."""
    X, y, bounds, h, post = _case(d)
    gp, _ = _device(X, y, h)
    rs = np.random.RandomState(4)
    A, B = rs.uniform(-2, 2, (17, d)), rs.uniform(-2, 2, (5, d))
    np.testing.assert_allclose(gp.kernel_matrix(A, B), G.kern_K(A, B, h['var'], h['ls'], h['bias']), rtol=1e-13, atol=1e-15)
    K = gp.kernel_matrix(A)
    np.testing.assert_allclose(K, G.kern_K(A, None, h['var'], h['ls'], h['bias']), rtol=1e-13, atol=1e-15)
    assert np.all(np.diag(K) == h['var'] + h['bias']) and K.shape == (17, 17)
    np.testing.assert_allclose(gp.kernel_matrix(X)[:5, :5], post.K[:5, :5], rtol=1e-13)
    gp.close()


@gpu
@pytest.mark.parametrize('d', [25, 65])
def test_cross_cov_and_maxvar(hip_ctx, d):
    """The oracles and tolerances of tests/test_maxvar_surfaces_gpu.py (cross covariance 1e-10 max(1, |cov|), query variance
    1e-8 (var + bias); MaxVar value 1e-7, gradient 1e-5 of the largest; a row against its own call 1e-12 / 1e-10)."""
    from test_maxvar_surfaces_gpu import _check_cross, _gauss_prior, _oracle_model, _oracle_surface
    X, y, bounds, h, post = _case(d)
    gp, _ = _device(X, y, h)
    rs = np.random.RandomState(d)
    P, Q = rs.uniform(-2, 2, (33, d)), rs.uniform(-2, 2, (17, d))
    Q[0], Q[-1] = P[0], X[N // 2]            # on an integration point, on an evidence point
    gp.set_integration_points(P)
    cov, var = _check_cross(gp, _oracle_model(X, post), h, P, Q, 'd = %d' % d)
    c1, v1 = gp.cross_cov(Q[16:17])
    assert np.max(np.abs(c1[:, 0] - cov[:, 16])) <= 1e-11 * max(1.0, np.max(np.abs(cov)))
    assert abs(v1[0] - var[16]) <= 1e-11 * (h['var'] + h['bias'])
    xs = _queries(X, 33)
    pdf, glog = _gauss_prior(xs)
    eps = float(np.percentile(y, 20))
    val, grad = gp.maxvar(xs, eps, pdf, glog)
    rval, rgrad = _oracle_surface(post, xs, eps, pdf, glog)
    _hold(d, 'MaxVar value', _scaled(val, rval), 1e-7)
    _hold(d, 'MaxVar gradient', _scaled(grad, rgrad), 1e-5)
    for r in (0, 15, 16, 32):
        v1, g1 = gp.maxvar(xs[r:r + 1], eps, pdf[r:r + 1], glog[r:r + 1])
        assert abs(v1[0, 0] - val[r, 0]) <= 1e-12 * np.max(np.abs(val)), 'row %d value' % r
        assert np.max(np.abs(g1[0] - grad[r])) <= 1e-10 * np.max(np.abs(grad)), 'row %d gradient' % r
    gp.close()


# ---- the limits of elfihip_gp_create -----------------------------------------------------------------------------------
@gpu
def test_limits_of_the_input_dimension(hip_ctx):
    from elfi_amd.gp import GPHandle
    for bad in (0, 257):
        with pytest.raises(ValueError, match='input dimension'):      # ELFIHIP_ERR_ARG
            GPHandle(bad, 8)
    d, n = 256, 8
    X, y, bounds, h, post = _case(d, n)
    gp, _ = _device(X[:n - 1], y[:n - 1], h, capacity=n)
    logz = gp.extend(X[n - 1:], y[n - 1:])
    _hold_factor(d, gp, logz, post, ' (capacity 8)')
    xs = _queries(X, 3)
    m, v, dmu, dvar = gp.predict_grad(xs)
    _hold_prediction(d, post, xs, m, v, dmu, dvar, tag=' (capacity 8)')
    val, grad = gp.lcb(xs, BETA)
    rval, rgrad = _lcb(post, xs, BETA)
    _hold(d, 'lcb (capacity 8)', _scaled(val, rval), 1e-8)
    _hold(d, 'lcb gradient (capacity 8)', _scaled(grad, rgrad), 1e-7)
    _, g = gp.nlml_grad()
    rg = post.log_marginal_grad()
    _hold(d, 'gradient of log Z (capacity 8)', np.max(np.abs(g - rg)) / np.max(np.abs(rg)), 1e-7)
    gp.close()
