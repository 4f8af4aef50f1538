"""The MaxVar family on the device across shapes: elfihip_gp_maxvar, elfihip_gp_set_integration_points,
elfihip_gp_cross_cov and elfihip_gp_expintvar (csrc/gp_predict.hip, csrc/special.hpp) against the CPU oracle and against
cancellation-free float64 forms of the surfaces, at the sizes tests/test_maxvar_gpu.py's one fixture never reaches: several
16-point passes and groups of passes, integration point counts on both sides of the kernels' strides (16, 32, 256), every
padding of d, evidence counts on both sides of the 128 blocks, point sets that change on a live GP.

Tolerances and where they come from
  the project's (tests/test_maxvar_gpu.py, tests/test_gp_gpu.py):
    MaxVar value vs oracle        1e-7 of max |value|
    MaxVar gradient vs oracle     1e-5 of max |gradient|
    cross covariance vs oracle    1e-10 max(1, max |cov|);  query variance 1e-8 (var + bias)
    ExpIntVar loss vs oracle      1e-7 of max |loss|
    a row vs the call with that row alone: value 1e-12 of scale, gradient 1e-10 (test_dense_form_many_points_in_rounds);
    a covariance column vs its own call 1e-11 max(1, max |cov|) (two groupings of one sum: the dense / streaming bound)
  derived:
    surface vs W = ndtr(z) ndtr(-z) - 2 owens_t(z, b) on the device's own prediction: 1e-12 p^2 absolute -- W <= 1/4, the
      quadrature's 1e-13 relative on T <= 1/4 and a few ulp of the erfc terms leave a margin of about 20;  no value below
      -1e-12 p^2;  gradient 1e-11 of the sum of the absolute terms of the chain rule (binary64 products and exp at |z| <= 38;
      1e-290 is added to that sum, since at |z| = 38 the terms are subnormal and carry no relative precision)
    one-hot ExpIntVar loss vs 2 owens_t(z_j, a_js): 1e-13 sum |w| (T <= 1/4 at 1e-13 relative: 5e-14, doubled for the
      rounding of the inputs)
    permuted rows: bit for bit (every query column is summed in an order that does not depend on its position)
  measured (tests/test_special_reference.py, against 50-digit values): SciPy's W form is off by 7.5e-17 absolute and
    owens_t by 4.2e-17, so the two derived tolerances are 1.3e4 and 1.2e3 times the measured error of their reference (the
    required factor is 4); the device quadrature's design error is 2.1e-14 on W and 1.1e-14 on T, 48 and 4.5 times below.

What these tests found: maxvar_kernel formed W as (Phi - Phi^2) - 2 T.  1 - Phi(z) has no digits left in the upper tail,
so W was right to 1e-16 absolute (the value test passes either way) but the gradient's term 2 p W (p grad log p) missed
its allowance: 1.3e-5 of the terms against 1e-11 (test_maxvar_epilogue_vs_float64_form).  The kernel now multiplies
Phi(z) by Phi(-z).

Deliberate one-line changes of csrc/gp_predict.hip, each rebuilt and run once against this file, and what failed:
  prior_pdf[s] -> prior_pdf[q] (maxvar_kernel)                  test_maxvar_surface_vs_oracle (every S > 16),
                                                                test_maxvar_epilogue_vs_float64_form, test_maxvar_prior_edge_rows
  (s / PC) * outsz -> 0 (expintvar_kernel)                      test_expintvar_loss_vs_oracle (every S > 16), the one-hot test
  integration points beyond the first 256 dropped               test_expintvar_loss_vs_oracle (every M > 256), the one-hot test
  col without s0 (cross_finish_kernel)                          test_cross_cov_vs_oracle and test_expintvar_loss_vs_oracle
                                                                (every S > 128), test_expintvar_clamps_a_negative_ratio
  2 T -> T (maxvar_kernel; the control)                         every surface test here and tests/test_maxvar_gpu.py
  m_pad of the previous point set (cross_cov_impl): not run -- with M = 1000 then 17 the product would walk a matrix of
    np x 32 doubles with a row stride of 1024, outside the allocation; test_integration_points_follow_the_state_of_the_gp
    is the test that changes m_pad on a live GP (1024 -> 32 -> 288) and compares with the oracle after each.

elfihip_gp_maxvar always runs the streaming form of the triangular products (it enqueues the 16-point passes itself and
never enters the dense predictor), so the surface is NOT run a second time under set_dense_threshold(64); the dense form
takes part where the epilogue test reads the prediction (predict_grad with S >= 112), under both thresholds.
"""
import numpy as np
import pytest
from scipy.special import ndtr, owens_t

import acquisition_oracle as AO
import gp_oracle as G
from test_gp_gpu import _problem
from test_maxvar import OracleModel

pytestmark = pytest.mark.gpu

_ORACLE_CACHE = {}


def _oracle_for(n, d, hyper=None):
    """(X, y, hyper, posterior) of the problem of this shape; one CPU posterior alive at a time (4096^2 LAPACK passes)."""
    key = (n, d, None if hyper is None else tuple(sorted(hyper.items())))
    if key not in _ORACLE_CACHE:
        _ORACLE_CACHE.clear()
        X, y, bounds = _problem(n, d, seed=n + d)
        h = hyper or G.default_hyper(bounds, y)
        _ORACLE_CACHE[key] = (X, y, h, G.Posterior(X, y, h['var'], h['ls'], h['bias'], h['noise']))
    return _ORACLE_CACHE[key]


def _device_gp(X, y, h, capacity=None):
    from elfi_amd.gp import GPHandle
    gp = GPHandle(X.shape[1], capacity or X.shape[0])
    gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    gp.set_data(X, y)
    gp.factorize()
    return gp


def _oracle_model(X, post):
    """tests/test_maxvar.py's OracleModel around a posterior that exists already."""
    om = OracleModel.__new__(OracleModel)
    om.post, om.X, om.input_dim, om.noise = post, X, X.shape[1], post.noise
    return om


def _gauss_prior(xs):
    """Product of Gaussians N(0.3, 3^2): density and gradient of its logarithm, in NumPy."""
    m, s = 0.3, 3.0
    pdf = np.prod(np.exp(-0.5 * ((xs - m) / s) ** 2) / (s * np.sqrt(2 * np.pi)), axis=1)
    return pdf, -(xs - m) / s ** 2


def _queries(X, S, seed):
    xs = np.random.RandomState(seed).uniform(-2, 2, (S, X.shape[1]))
    xs[0] = X[len(X) // 3]          # on an evidence point
    xs[-1] = 6.0                    # far outside the evidence (S = 1: this one)
    return xs


def _oracle_surface(post, xs, eps, pdf, glog):
    val, grad = [], []
    for lo in range(0, len(xs), 256):      # (the oracle's gradient builds an (S, n, d) array)
        sl = slice(lo, lo + 256)
        mean, var = post.predict(xs[sl], noiseless=True)
        gm, gv = post.predictive_gradients(xs[sl])
        val.append(AO.maxvar_value(mean, var, post.noise, eps, pdf[sl]))
        grad.append(AO.maxvar_gradient(mean, var, gm, gv, post.noise, eps, pdf[sl], glog[sl]))
    return np.concatenate(val), np.concatenate(grad)


def _boundary_rows(S):
    """Rows on both sides of every kind of boundary: passes of 16, groups of 8 passes, the last pass."""
    rows = {0, S - 1, S // 2}
    for b in (16, 32, 128, 256, 16 * ((S - 1) // 16), 128 * ((S - 1) // 128)):
        rows.update((b - 1, b, b + 1))
    return sorted(r for r in rows if 0 <= r < S)


# every S in {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257, 1000, 4097, 9001}, every d in {1, 2, 3, 7, 8, 10, 20, 23, 30},
# every n in {5, 128, 129, 300, 1000, 2048, 4096}; n = 2048 and 4096 with S >= 256; grouped by (n, d) for the oracle cache
SURFACE_CASES = [
    (5, 1, 1), (5, 1, 17), (5, 2, 15), (5, 3, 16), (5, 7, 33), (5, 10, 255),
    (128, 2, 31), (128, 3, 1000), (128, 7, 32), (128, 8, 33), (128, 23, 65),
    (129, 1, 255), (129, 3, 63), (129, 10, 64), (129, 20, 65), (129, 30, 15),
    (300, 2, 257), (300, 2, 9001), (300, 7, 4097), (300, 8, 63), (300, 23, 17), (300, 30, 16),
    (1000, 1, 31), (1000, 2, 64), (1000, 3, 15), (1000, 8, 255), (1000, 10, 1000), (1000, 20, 257), (1000, 23, 33),
    (1000, 30, 65),
    (2048, 2, 1), (2048, 3, 4097), (2048, 7, 64), (2048, 10, 257), (2048, 20, 32),
    (4096, 2, 17), (4096, 8, 63), (4096, 10, 257), (4096, 10, 1000), (4096, 23, 16),
]


@pytest.mark.parametrize('n,d,S', SURFACE_CASES)
def test_maxvar_surface_vs_oracle(hip_ctx, n, d, S):
    """(a) value and gradient end to end: acquisition_oracle.maxvar_value / maxvar_gradient over gp_oracle.Posterior."""
    X, y, h, post = _oracle_for(n, d)
    gp = _device_gp(X, y, h)
    xs = _queries(X, S, seed=S + d)
    pdf, glog = _gauss_prior(xs)
    eps = float(np.percentile(y, 20))
    val, grad = gp.maxvar(xs, eps, pdf, glog)
    rval, rgrad = _oracle_surface(post, xs, eps, pdf, glog)
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    verr = np.max(np.abs(val - rval)) / np.max(np.abs(rval))
    gerr = np.max(np.abs(grad - rgrad)) / np.max(np.abs(rgrad))
    print('n %d d %d S %d: value %.3g gradient %.3g' % (n, d, S, verr, gerr))
    assert verr <= 1e-7, 'value: %g of the largest' % verr
    assert gerr <= 1e-5, 'gradient: %g of the largest' % gerr
    # every row equals the call with that row alone
    vs, gs = np.max(np.abs(val)), np.max(np.abs(grad))
    for r in _boundary_rows(S):
        v1, g1 = gp.maxvar(xs[r:r + 1], eps, pdf[r:r + 1], glog[r:r + 1])
        assert abs(v1[0, 0] - val[r, 0]) <= 1e-12 * vs, 'row %d value' % r
        assert np.max(np.abs(g1[0] - grad[r])) <= 1e-10 * gs, 'row %d gradient' % r
    # permuting the rows together with their prior arrays permutes the outputs, bit for bit
    perm = np.random.RandomState(S).permutation(S)
    vp, gpm = gp.maxvar(xs[perm], eps, pdf[perm], glog[perm])
    assert np.array_equal(vp, val[perm]) and np.array_equal(gpm, grad[perm]), \
        'permutation: value %g gradient %g' % (np.max(np.abs(vp - val[perm])), np.max(np.abs(gpm - grad[perm])))
    gp.close()


# ---- (b) the epilogue alone ------------------------------------------------------------------------------------------
Z_TARGETS = [0.0] + [s * v for v in (1e-3, 1.0, 3.0, 6.0, 9.0, 20.0, 37.0, 38.0) for s in (1.0, -1.0)]


def _surface_f64(mu, var, dmu, dvar, eps, s2n, pdf, glog):
    """value, gradient and the gradient's allowance scale from a prediction, by the kernel's header formulas in float64
    with SciPy's special functions."""
    m, v = mu[:, 0], var[:, 0]
    sv, sb = s2n + v, s2n + 2.0 * v
    sdev = np.sqrt(sv)
    z = (eps - m) / sdev
    b = np.sqrt(s2n) / np.sqrt(sb)
    Pz, Pm, pz = ndtr(z), ndtr(-z), np.exp(-0.5 * z * z) / np.sqrt(2 * np.pi)
    T = owens_t(z, b)
    W = Pz * Pm - 2.0 * T
    dT_dh = -pz * (ndtr(z * b) - 0.5)
    dT_da = np.exp(-0.5 * z * z * (1.0 + b * b)) / (2 * np.pi * (1.0 + b * b))
    dW_dz = (1.0 - 2.0 * Pz) * pz - 2.0 * dT_dh
    dW_dz_abs = np.abs(1.0 - 2.0 * Pz) * pz + 2.0 * np.abs(dT_dh)
    dz_dm, dz_dv, db_dv = -1.0 / sdev, -(eps - m) / (2.0 * sv * sdev), -np.sqrt(s2n) / (sb * np.sqrt(sb))
    c = lambda a: a[:, None]
    dz = c(dz_dm) * dmu + c(dz_dv) * dvar
    dz_abs = np.abs(c(dz_dm) * dmu) + np.abs(c(dz_dv) * dvar)
    dW = c(dW_dz) * dz - 2.0 * c(dT_da) * (c(db_dv) * dvar)
    dW_abs = c(dW_dz_abs) * dz_abs + 2.0 * c(dT_da) * np.abs(c(db_dv) * dvar)
    p = c(pdf)
    with np.errstate(invalid='ignore', over='ignore'):
        val = pdf * pdf * W
        grad = 2.0 * p * c(W) * (p * glog) + p * p * dW
        scale = 2.0 * p * p * c(Pz * Pm + 2.0 * T) * np.abs(glog) + p * p * dW_abs
    return val, grad, scale, z, b


EPILOGUE_GPS = [
    # (n, d, hyper or None, S): b = sqrt(s_n / (s_n + 2 v)) from ~1e-3 (tiny noise, far from the evidence) to 1 - 1e-9
    (300, 2, dict(var=1.0, ls=0.5, bias=0.25, noise=1e-6), 40),
    (300, 3, None, 130),                                             # (S >= 112: predict_grad takes the dense form)
    (129, 2, dict(var=1.0, ls=1.0, bias=0.25, noise=1e3), 33),
    (200, 7, dict(var=1.0, ls=2.0, bias=0.25, noise=1e9), 17),
]


def test_maxvar_epilogue_vs_float64_form(hip_ctx):
    """(b) mu, var and their gradients from the device's own predict_grad; the surface from them in float64."""
    b_seen, z_seen = [], []
    for n, d, hyper, S in EPILOGUE_GPS:
        X, y, bounds = _problem(n, d, seed=n + d)
        h = hyper or G.default_hyper(bounds, y)
        gp = _device_gp(X, y, h)
        xs = _queries(X, S, seed=5)
        xs[1] = X[0] + 1e-9
        pdf, glog = _gauss_prior(xs)
        for thr in (1 << 40, 64):
            try:
                gp.set_dense_threshold(thr)
                mu, var, dmu, dvar = gp.predict_grad(xs)
            finally:
                gp.set_dense_threshold(0)
            sdev = np.sqrt(h['noise'] + var[:, 0])
            for k, z0 in enumerate(Z_TARGETS):
                anchor = k % S
                eps = float(mu[anchor, 0] + z0 * sdev[anchor])      # z = z0 at the anchor (z0 = 0: exactly)
                val, grad = gp.maxvar(xs, eps, pdf, glog)
                rval, rgrad, scale, z, b = _surface_f64(mu, var, dmu, dvar, eps, h['noise'], pdf, glog)
                if z0 == 0.0:
                    assert z[anchor] == 0.0
                b_seen.append(b)
                z_seen.append(z)
                assert not np.any(np.isnan(val)) and not np.any(np.isnan(grad))
                verr = np.max(np.abs(val[:, 0] - rval) / pdf ** 2)
                assert verr <= 1e-12, 'value: %g p^2 (n %d, z0 %g)' % (verr, n, z0)
                assert np.all(val[:, 0] >= -1e-12 * pdf ** 2)
                gerr = np.max(np.abs(grad - rgrad) / (scale + 1e-290))     # (|z| = 38: phi(z) = 1e-314 is subnormal)
                assert gerr <= 1e-11, 'gradient: %g of its terms (n %d, z0 %g)' % (gerr, n, z0)
        gp.close()
    b_all, z_all = np.concatenate(b_seen), np.concatenate(z_seen)
    print('b in [%g, 1 - %g], z in [%g, %g]' % (b_all.min(), 1 - b_all.max(), z_all.min(), z_all.max()))
    assert b_all.min() <= 2e-3 and b_all.max() >= 1.0 - 2e-9
    assert z_all.min() <= -38.0 + 1e-9 and z_all.max() >= 38.0 - 1e-9
    for v in (1e-3, 1.0, 3.0, 6.0, 9.0, 20.0, 37.0):
        assert np.min(np.abs(np.abs(z_all) - v)) <= 1e-9 * max(1.0, v)


def test_maxvar_prior_edge_rows(hip_ctx):
    """prior_pdf = 0 with a finite gradient of the log density: exactly 0; +-inf in prior_grad_logpdf: the NaN / inf
    pattern of the formula  2 p W (p g) + p^2 dW  evaluated in IEEE arithmetic."""
    n, d, S = 300, 3, 37
    X, y, bounds = _problem(n, d, seed=n + d)
    h = G.default_hyper(bounds, y)
    gp = _device_gp(X, y, h)
    xs = _queries(X, S, seed=9)
    pdf, glog = _gauss_prior(xs)
    zero_rows = [0, 15, 16, 20, 36]
    pdf[zero_rows] = 0.0
    glog[3, 0], glog[17, 1], glog[33, 2] = np.inf, -np.inf, np.inf          # p > 0
    glog[20, 1], glog[36, 0] = np.inf, -np.inf                              # p = 0: 0 * inf
    eps = float(np.percentile(y, 20))
    val, grad = gp.maxvar(xs, eps, pdf, glog)
    mu, var, dmu, dvar = gp.predict_grad(xs)
    rval, rgrad, _, _, _ = _surface_f64(mu, var, dmu, dvar, eps, h['noise'], pdf, glog)
    for r in (0, 15, 16):
        assert val[r, 0] == 0.0 and np.all(grad[r] == 0.0)
    assert np.all(val[zero_rows, 0] == 0.0) and not np.any(np.isnan(val))
    assert np.array_equal(np.isnan(grad), np.isnan(rgrad))
    assert np.array_equal(np.isinf(grad), np.isinf(rgrad))
    inf = np.isinf(rgrad)
    assert np.array_equal(np.sign(grad[inf]), np.sign(rgrad[inf]))
    assert np.isnan(grad[20, 1]) and np.isnan(grad[36, 0]) and inf[3, 0] and inf[17, 1] and inf[33, 2]
    fin = np.isfinite(rgrad)
    assert np.max(np.abs(grad[fin] - rgrad[fin])) <= 1e-10 * np.max(np.abs(rgrad[fin]))
    gp.close()


# ---- (c) cross covariance --------------------------------------------------------------------------------------------
# every M in {1, 15, 16, 17, 31, 32, 33, 100, 255, 256, 257, 1000}, S in {1, 16, 17, 127, 128, 129, 300, 1000},
# d in {1, 2, 5, 10, 23}, n in {5, 128, 129, 1000, 4096}
CROSS_CASES = [
    (5, 1, 1, 1), (5, 2, 15, 16), (128, 2, 16, 17), (128, 1, 17, 1000), (128, 5, 17, 127), (129, 5, 31, 128),
    (129, 10, 32, 129), (129, 23, 256, 16), (1000, 10, 33, 300), (1000, 2, 100, 1000), (1000, 23, 255, 1),
    (1000, 5, 1000, 1000), (4096, 10, 257, 300), (4096, 10, 1000, 129),
]


def _points(d, M, seed):
    return np.random.RandomState(seed).uniform(-2, 2, (M, d))


def _check_cross(gp, om, h, P, Q, what=''):
    cov, var = gp.cross_cov(Q)
    om.set_integration_points(P)
    rcov, rvar = om.cross_cov(Q)
    assert cov.shape == (len(P), len(Q)) and var.shape == (len(Q),)
    cerr = np.max(np.abs(cov - rcov)) / max(1.0, np.max(np.abs(rcov)))
    verr = np.max(np.abs(var - rvar)) / (h['var'] + h['bias'])
    assert cerr <= 1e-10, '%s covariance: %g' % (what, cerr)
    assert verr <= 1e-8, '%s variance: %g' % (what, verr)
    return cov, var


@pytest.mark.parametrize('n,d,M,S', CROSS_CASES)
def test_cross_cov_vs_oracle(hip_ctx, n, d, M, S):
    X, y, h, post = _oracle_for(n, d)
    gp = _device_gp(X, y, h)
    om = _oracle_model(X, post)
    P, Q = _points(d, M, seed=M), _points(d, S, seed=1000 + S)
    Q[0] = P[0]                                  # a query point on an integration point
    if S > 1:
        Q[-1] = X[n // 2]                        # ... and one on an evidence point
    gp.set_integration_points(P)
    cov, var = _check_cross(gp, om, h, P, Q, 'P x Q')
    top = max(1.0, np.max(np.abs(cov)))
    # column s is the single-point call with Q[s]
    for s in sorted({0, S - 1, S // 2} | {c for b in (16, 32, 128, 256) for c in (b - 1, b, b + 1) if c < S}):
        c1, v1 = gp.cross_cov(Q[s:s + 1])
        assert np.max(np.abs(c1[:, 0] - cov[:, s])) <= 1e-11 * top, 'column %d' % s
        assert abs(v1[0] - var[s]) <= 1e-11 * (h['var'] + h['bias'])
    # the point set against itself: symmetric, the noiseless variance on the diagonal
    cpp, vpp = _check_cross(gp, om, h, P, P, 'P x P')
    assert np.max(np.abs(cpp - cpp.T)) <= 1e-10 * max(1.0, np.max(np.abs(cpp)))
    assert np.max(np.abs(np.diag(cpp) - vpp)) <= 1e-10 * max(1.0, np.max(np.abs(cpp)))
    gp.close()


def test_integration_points_follow_the_state_of_the_gp(hip_ctx):
    """A new point set on a live GP (other M, other m_pad: freed and allocated again), new evidence by bordering inside a
    128 block and across one, new hyper-parameters: a stale point set raises, the set again gives the oracle's numbers."""
    n0, d = 100, 3
    X, y, bounds = _problem(200, d, seed=42)
    h = G.default_hyper(bounds, y)
    gp = _device_gp(X[:n0], y[:n0], h, capacity=300)
    Q = _points(d, 45, seed=2)
    sets = {M: _points(d, M, seed=M) for M in (1000, 17, 257)}

    def oracle(n, hh):
        return _oracle_model(X[:n], G.Posterior(X[:n], y[:n], hh['var'], hh['ls'], hh['bias'], hh['noise']))

    om = oracle(n0, h)
    for M in (1000, 17, 257):
        gp.set_integration_points(sets[M])
        _check_cross(gp, om, h, sets[M], Q, 'M = %d' % M)
    P = sets[257]
    w = np.random.RandomState(1).uniform(0.1, 1.0, len(P))
    n = n0
    for k in (5, 30):                                   # 100 -> 105 inside the block, 105 -> 135 across 128
        gp.extend(X[n:n + k], y[n:n + k])
        n += k
        with pytest.raises(RuntimeError):
            gp.cross_cov(Q)
        with pytest.raises(RuntimeError):
            gp.expintvar(Q, 0.5, w, np.zeros(len(P)), np.ones(len(P)))
        om = oracle(n, h)
        gp.set_integration_points(P)
        _check_cross(gp, om, h, P, Q, 'n = %d' % n)
    h2 = dict(h, ls=0.8 * h['ls'], noise=2.0 * h['noise'])
    gp.set_hyper(h2['var'], h2['ls'], h2['bias'], h2['noise'])
    gp.factorize()
    with pytest.raises(RuntimeError):
        gp.cross_cov(Q)
    gp.set_integration_points(P)
    _check_cross(gp, oracle(n, h2), h2, P, Q, 'new hyper-parameters')
    # no points: maxvar answers with nothing, the others report the argument (include/elfihip.h)
    e = np.empty((0, d))
    val, grad = gp.maxvar(e, 0.5, np.empty(0), e)
    assert val.shape == (0, 1) and grad.shape == (0, d)
    with pytest.raises(ValueError):
        gp.cross_cov(e)
    with pytest.raises(ValueError):
        gp.expintvar(e, 0.5, w, np.zeros(len(P)), np.ones(len(P)))
    with pytest.raises(ValueError):
        gp.set_integration_points(e)
    _check_cross(gp, oracle(n, h2), h2, P, Q, 'after the refused calls')     # the refused set left the old one in place
    gp.close()


# ---- (d) ExpIntVar loss ----------------------------------------------------------------------------------------------
# every M in {1, 17, 255, 256, 257, 1000, 3000}, every S in {1, 15, 16, 17, 33, 257, 1000}
LOSS_CASES = [(300, 2, 1, 1), (300, 2, 17, 15), (300, 5, 255, 16), (300, 2, 256, 17), (1000, 10, 257, 33),
              (300, 3, 1000, 257), (300, 2, 17, 1000), (300, 2, 3000, 33), (129, 2, 3000, 17)]


@pytest.mark.parametrize('n,d,M,S', LOSS_CASES)
def test_expintvar_loss_vs_oracle(hip_ctx, n, d, M, S):
    X, y, h, post = _oracle_for(n, d)
    gp = _device_gp(X, y, h)
    om = _oracle_model(X, post)
    P, Q = _points(d, M, seed=M + 1), _points(d, S, seed=2000 + S)
    Q[0] = P[M // 2]
    w = np.random.RandomState(M).uniform(0.05, 1.0, M)
    mean_int, var_int = (a[:, 0] for a in post.predict(P, noiseless=True))
    eps = float(np.percentile(y, 20))
    gp.set_integration_points(P)
    loss = gp.expintvar(Q, eps, w, mean_int, var_int)
    om.set_integration_points(P)
    ref = om.expintvar_loss(Q, eps, w, mean_int, var_int)
    assert loss.shape == (S,) and np.all(np.isfinite(loss))
    err = np.max(np.abs(loss - ref)) / np.max(np.abs(ref))
    print('n %d d %d M %d S %d: loss %.3g' % (n, d, M, S, err))
    assert err <= 1e-7, 'loss: %g of the largest' % err
    gp.close()


def test_expintvar_one_hot_weights_give_owens_t(hip_ctx):
    """w = e_j: loss_s = 2 T(z_j, a_js), with a_js in float64 from the device's own covariance.  j on both sides of the
    256-thread stride over the integration points, z_j over the grid of the epilogue test."""
    n, d, M, S = 300, 2, 1000, 33
    X, y, bounds = _problem(n, d, seed=n + d)
    h = G.default_hyper(bounds, y)
    gp = _device_gp(X, y, h)
    P, Q = _points(d, M, seed=3), _points(d, S, seed=4)
    P[255] = 5.0                                  # an integration point far from the evidence: v >> s_n, small a on itself
    Q[:4] = P[[0, 255, 256, M - 1]]
    Q[-1] = 6.0                                   # far from everything: covariance ~ 0, a ~ 1
    gp.set_integration_points(P)
    cov, var_q = gp.cross_cov(Q)
    _, var_int = gp.predict(P, noiseless=True)
    var_int = var_int[:, 0]
    s2n, eps = h['noise'], 0.7
    worst, a_lo, a_hi = 0.0, 1.0, 0.0
    for j in (0, 255, 256, M - 1):
        A = s2n + var_int[j]
        dl = cov[j] * cov[j] / (s2n + var_q)
        a = np.sqrt(np.maximum((A - dl) / (A + dl), 0.0))
        a_lo, a_hi = min(a_lo, a.min()), max(a_hi, a.max())
        w = np.zeros(M)
        w[j] = 1.0
        for z0 in Z_TARGETS:
            mean_int = np.random.RandomState(j).uniform(-1, 1, M)
            mean_int[j] = eps - z0 * np.sqrt(A)
            z = (eps - mean_int[j]) / np.sqrt(A)
            loss = gp.expintvar(Q, eps, w, mean_int, var_int)
            ref = 2.0 * owens_t(z, a)
            assert not np.any(np.isnan(loss))
            worst = max(worst, np.max(np.abs(loss - ref)))
            assert np.max(np.abs(loss - ref)) <= 1e-13, 'j %d z %g: %g' % (j, z, np.max(np.abs(loss - ref)))
    print('one-hot loss: worst %.3g, a in [%g, %g]' % (worst, a_lo, a_hi))
    assert a_hi >= 0.99 and a_lo <= 0.9
    gp.close()


def test_expintvar_clamps_a_negative_ratio(hip_ctx):
    """(A - c^2 / den) / (A + c^2 / den) below 0 -- a variance of the integration point that is smaller than the
    covariance allows, which rounding produces when Q lies on the point and the noise is tiny -- is T(z, 0) = 0, not NaN."""
    n, d, M = 300, 2, 300
    X, y, bounds = _problem(n, d, seed=n + d)
    h = G.default_hyper(bounds, y)
    gp = _device_gp(X, y, h)
    P = np.random.RandomState(6).uniform(4.0, 6.0, (M, d))        # far from the evidence: v ~ var + bias >> noise
    gp.set_integration_points(P)
    cov, var_q = gp.cross_cov(P)
    assert np.all(np.diag(cov) ** 2 / (h['noise'] + var_q) > 1.7 * h['noise'])
    for j in (0, 255, 256, M - 1):
        w = np.zeros(M)
        w[j] = 1.0
        loss = gp.expintvar(P, 0.5, w, np.zeros(M), np.zeros(M))    # var_int = 0: A = s_n < c^2 / den in column j
        assert not np.any(np.isnan(loss)) and loss[j] == 0.0 and np.all(loss >= 0.0)
    gp.close()
    # the natural occurrence: tiny noise, the candidates on the integration points, consistent variances
    ht = dict(var=1.0, ls=0.5, bias=0.25, noise=1e-10)
    gp = _device_gp(X, y, ht)
    Pn = np.concatenate([X[:40], _points(d, 60, seed=8)])
    gp.set_integration_points(Pn)
    mean_int, var_int = (a[:, 0] for a in gp.predict(Pn, noiseless=True))
    loss = gp.expintvar(Pn, 0.5, np.ones(len(Pn)), mean_int, np.maximum(var_int, 0.0))
    assert np.all(np.isfinite(loss)) and np.all(loss >= 0.0) and np.all(loss <= 0.5 * len(Pn))
    gp.close()
