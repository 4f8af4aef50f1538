"""GPU: log-marginal gradient, K^-1 and the hyper-parameter MAP fit vs the CPU oracle.

Tolerances: gradient of log Z w.r.t. (var, ls, bias, noise) relative 1e-7 of the largest
component (sums of n^2 terms with cancellation between alpha alpha^T and K^-1); K^-1 relative
1e-8.  The optimiser is "parity unpinned" (oracle/gp_hyper_oracle.py): the GPU run and the CPU
restatement start from the same point and must reach the same MAP objective within 1e-5
relative and hyper-parameters within 1 %; SCG amplifies last-digit gradient differences through
its one-sided curvature estimate (sigma = 1e-7), so trajectories are not compared point by point.
"""
import numpy as np
import pytest

import gp_hyper_oracle as HO
import gp_oracle as G

pytestmark = pytest.mark.gpu


def _fit(n, d, seed, hyper=None):
    from elfi_amd.gp import GPHandle
    X, y, bounds = G.synthetic_gp_problem(n, d, seed=seed)
    h = hyper or G.default_hyper(bounds, y)
    gp = GPHandle(d, n)
    gp.set_hyper(h['var'], h['ls'], h['bias'], h['noise'])
    gp.set_data(X, y)
    logz = gp.factorize()
    return gp, logz, G.Posterior(X, y, h['var'], h['ls'], h['bias'], h['noise']), (X, y, bounds)


def _scaled_hyper(n, d, seed):
    """The default hyper-parameters with the lengthscale multiplied by sqrt(d / 2): evidence points in [-2, 2]^d stay
    correlated at any d (tests/test_gp_dimensions_gpu.py), so every coordinate of X reaches the gradient."""
    X, y, bounds = G.synthetic_gp_problem(n, d, seed=seed)
    h = dict(G.default_hyper(bounds, y))
    h['ls'] *= np.sqrt(d / 2.0)
    return h


# (400, 70) with the default lengthscale 4/3: the largest off-diagonal k / var is 4e-12, d log Z / d ls 2.7e-11 -- K is the
# identity to rounding and X does not matter; the case stays, and the scaled one beside it is the test of
# kinv_grad_kernel's global-memory path (dp >= 48)
@pytest.mark.parametrize('n,d,scaled', [pytest.param(n, d, False, id='%d-%d' % (n, d)) for n, d in
                                        [(7, 1), (100, 2), (128, 3), (257, 2), (700, 10), (1300, 20), (400, 70)]]
                         + [pytest.param(400, 70, True, id='400-70-scaled-lengthscale')])
def test_log_marginal_gradient_vs_oracle(hip_ctx, n, d, scaled):
    gp, logz, ref, _ = _fit(n, d, seed=n + d, hyper=_scaled_hyper(n, d, n + d) if scaled else None)
    lz, g = gp.nlml_grad()
    assert lz == logz
    assert abs(lz - ref.log_marginal) <= 1e-9 * abs(ref.log_marginal)
    rg = ref.log_marginal_grad()
    assert np.max(np.abs(g - rg)) <= 1e-7 * np.max(np.abs(rg)), (g, rg)


def test_gradient_with_other_hyperparameters(hip_ctx):
    h = dict(var=1.0, ls=1.0, bias=1.0, noise=0.05)   # the reference's initial kernel values
    gp, logz, ref, _ = _fit(500, 4, seed=3, hyper=h)
    _, g = gp.nlml_grad()
    rg = ref.log_marginal_grad()
    assert np.max(np.abs(g - rg)) <= 1e-7 * np.max(np.abs(rg))
    # the gradient is the derivative of what factorize() returns
    eps = 1e-5
    for i, k in enumerate(('var', 'ls', 'bias', 'noise')):
        hp, hm = dict(h), dict(h)
        hp[k] += eps
        hm[k] -= eps
        gp.set_hyper(hp['var'], hp['ls'], hp['bias'], hp['noise'])
        fp = gp.factorize()
        gp.set_hyper(hm['var'], hm['ls'], hm['bias'], hm['noise'])
        fm = gp.factorize()
        fd = (fp - fm) / (2 * eps)
        assert abs(fd - g[i]) <= 1e-5 * (1 + abs(g[i])), (k, fd, g[i])


def test_kinv_vs_oracle(hip_ctx):
    gp, _, ref, _ = _fit(300, 3, seed=9)
    gp.form_kinv()
    Ki = gp.get(5)
    assert np.max(np.abs(Ki - ref.Kinv)) <= 1e-8 * np.max(np.abs(ref.Kinv))
    assert np.array_equal(Ki, Ki.T)


def test_optimize_vs_oracle(hip_ctx):
    from elfi_amd import HipGPRegression
    from elfi_amd import hyperopt as H
    X, y, bounds = G.synthetic_gp_problem(200, 2, seed=5)
    names = ['t1', 't2']
    m = HipGPRegression(names, bounds=dict(zip(names, bounds)))
    m.update(X, y)
    assert m._hyper == G.initial_hyper(y)
    pri = G.default_priors(bounds, y)
    assert {k: tuple(v) for k, v in m._priors.items()} == {k: (pytest.approx(v[0]), pytest.approx(v[1]))
                                                          for k, v in pri.items()}
    obj = H.MarginalObjective(m)
    ref_obj = HO.MapObjective(X, y, pri)
    phi0 = H.logexp_inv(np.array([m._hyper[k] for k in H.NAMES]))
    f0, g0 = obj.f(phi0), obj.grad(phi0)
    assert abs(f0 - ref_obj.value(phi0)) <= 1e-9 * abs(f0)
    assert np.max(np.abs(g0 - ref_obj.gradient(phi0))) <= 1e-7 * np.max(np.abs(g0))
    m.optimize()
    info = m._opt_info
    href, iref = HO.optimize(X, y, G.initial_hyper(y), pri, max_iters=50)
    f_gpu, f_cpu = info['objective'][-1], iref['objective'][-1]
    assert f_gpu < f0 - 1.0, 'optimisation must improve the MAP objective'
    assert abs(f_gpu - f_cpu) <= 1e-5 * abs(f_cpu), (f_gpu, f_cpu)
    for k in H.NAMES:
        assert abs(m._hyper[k] - href[k]) <= 1e-2 * href[k], (k, m._hyper[k], href[k])
    # the model is refitted at the optimum
    ref = G.Posterior(X, y, **m._hyper)
    xs = np.random.RandomState(0).uniform(-2, 2, (5, 2))
    np.testing.assert_allclose(m.predict(xs)[0], ref.predict(xs)[0], rtol=1e-7)
    assert m.noise == m._hyper['noise']
    assert 'rbf.lengthscale' in str(m)


def test_update_with_optimize_flag(hip_ctx):
    from elfi_amd import HipGPRegression
    X, y, bounds = G.synthetic_gp_problem(120, 2, seed=8)
    m = HipGPRegression(['a', 'b'], bounds={'a': bounds[0], 'b': bounds[1]}, max_opt_iters=10)
    m.update(X[:100], y[:100], optimize=True)
    h1 = dict(m._hyper)
    assert h1 != G.initial_hyper(y[:100])
    m.update(X[100:], y[100:])          # no optimisation: hyper-parameters carried over (:306-310)
    assert m._hyper == h1 and m.n_evidence == 120


def test_map_search_reaches_the_reference_s_published_optimum(hip_ctx):
    """a10 pinned: on the evidence of the documented BOLFI run (tests/golden/bolfi_doc_run.npz; the CPU oracle
    reproduces the print-out of docs/usage/BOLFI.rst:144-153 digit for digit, tests/test_oracle_pinning_gp.py) the
    device MAP search, started where the run's last search started, must end at the PRINTED hyper-parameters and
    objective.  SCG stops on a relative objective change of 1e-6, so the end points of two correct implementations
    agree to about the square root of that in the well-determined directions."""
    import os
    from conftest import GOLDEN
    from elfi_amd import HipGPRegression
    from elfi_amd import hyperopt as H
    g = np.load(os.path.join(GOLDEN, 'bolfi_doc_run.npz'))
    names = ['t1', 't2']
    m = HipGPRegression(names, bounds={'t1': (-2, 2), 't2': (-1, 1)})
    m.update(g['X'], g['Y'])
    m._priors = {k: (float(g['priors'][i, 0]), float(g['priors'][i, 1])) for i, k in enumerate(('var', 'ls', 'bias'))}
    m._hyper = dict(zip(H.NAMES, (float(v) for v in g['hyper_start'])))
    m._refit()
    obj = H.MarginalObjective(m)
    printed = g['hyper_printed']
    f_printed = obj.f(H.logexp_inv(printed))
    # the device objective at the printed values is the printed objective (151.866...)
    assert abs(f_printed - float(g['objective_printed_in_doc'])) <= 1e-6 * 151.87, f_printed
    assert abs(f_printed - float(g['objective_at_printed'])) <= 1e-9 * 151.87
    m.optimize()
    got = np.array([m._hyper[k] for k in H.NAMES])
    f_got = m._opt_info['objective'][-1]
    assert abs(f_got - float(g['objective_printed_in_doc'])) <= 1e-6 * 151.87, (f_got, m._opt_info['status'])
    np.testing.assert_allclose(got[[0, 1, 3]], printed[[0, 1, 3]], rtol=2e-3)
    np.testing.assert_allclose(got[2], printed[2], rtol=5e-2)          # the flat bias direction
    # and the gradient of the device objective vanishes at the printed optimum to the search's own tolerance
    assert np.max(np.abs(obj.grad(H.logexp_inv(printed)))) <= 5e-3


@pytest.mark.parametrize('optimizer', ['lbfgsb', 'bfgs', 'tnc', 'simplex'])
def test_other_optimizers_reach_the_map_objective(hip_ctx, optimizer):
    """GPyRegression(optimizer=...) hands the name to GPy's model.optimize (gpy_regression.py:30,321); besides 'scg' the
    SciPy-backed searches run on the same device objective.  They must improve the MAP objective and -- given enough
    iterations -- end at (or below) the optimum the default search finds."""
    from elfi_amd import HipGPRegression
    X, y, bounds = G.synthetic_gp_problem(200, 2, seed=5)
    names = ['t1', 't2']
    ref_m = HipGPRegression(names, bounds=dict(zip(names, bounds)), max_opt_iters=200)
    ref_m.update(X, y, optimize=True)
    f_scg = ref_m._opt_info['objective'][-1]
    m = HipGPRegression(names, bounds=dict(zip(names, bounds)), optimizer=optimizer,
                        max_opt_iters=2000 if optimizer == 'simplex' else 400)
    m.update(X, y)
    from elfi_amd import hyperopt as H
    f0 = H.MarginalObjective(m).f(H.logexp_inv(np.array([m._hyper[k] for k in H.NAMES])))
    m.optimize()
    f1 = m._opt_info['objective'][-1]
    assert f1 < f0 - 1.0
    assert f1 <= f_scg + 1e-3 * abs(f_scg), (optimizer, f1, f_scg)
    post = G.Posterior(X, y, **m._hyper)                       # refitted at the optimum
    xs = np.random.RandomState(0).uniform(-2, 2, (5, 2))
    np.testing.assert_allclose(m.predict(xs)[0], post.predict(xs)[0], rtol=1e-7)
    with pytest.raises(ValueError):
        bad = HipGPRegression(names, bounds=dict(zip(names, bounds)), optimizer='nope')
        bad.update(X, y, optimize=True)


@pytest.mark.timeout(1200)
def test_whole_scg_search_at_n_2048_next_to_the_oracle(hip_ctx):
    """a10 at scale: ONE whole MAP search of the hyper-parameters (SCG, gpy_regression.py:317-323) on the device next to
    the oracle's SCG, at the size a configs[2] run searches at -- n = 2048, d = 2, evidence of the MA2 model as BOLFI
    collects it (parameters from the example's priors, y = log distance of the simulated autocovariances to the observed
    ones).  Every evaluation is a device rebuild + K^-1 gradient on one side, a LAPACK Cholesky + dense gradient on the
    other: the same number of iterations and of evaluations, the same stopping reason, per-iteration objective values
    within 5e-6 of the search's total decrease (SCG takes its curvature from a gradient difference over a step of 1e-7:
    the 1e-9 agreement of the two gradients reaches the step lengths as 1e-2 x 1e-4 -- measured 1e-6), and end points that
    agree as far as SCG's own stopping rule determines them (same objective value under the oracle; parameters to 5e-3)."""
    from elfi_amd import HipGPRegression
    from elfi_amd import hyperopt as H
    rs = np.random.RandomState(4)
    n = 2048
    u = rs.uniform(size=n)                                   # elfi/examples/ma2.py: CustomPrior1 (b = 2), CustomPrior2 (a = 1)
    t1 = np.where(u < 0.5, np.sqrt(2. * u) * 2 - 2, -np.sqrt(2. * (1. - u)) * 2 + 2)
    t2 = rs.uniform(-1.0, 1.0, n)                            # (inside the bounds; the triangle's corners do not matter here)
    w = rs.randn(n, 102)
    x = w[:, 2:] + t1[:, None] * w[:, 1:-1] + t2[:, None] * w[:, :-2]
    S1, S2 = np.mean(x[:, 1:] * x[:, :-1], axis=1), np.mean(x[:, 2:] * x[:, :-2], axis=1)
    y = np.log(np.sqrt((S1 - 0.55) ** 2 + (S2 - 0.18) ** 2))[:, None]
    X = np.column_stack([t1, t2])
    bounds = [(-2, 2), (-1, 1)]
    m = HipGPRegression(['t1', 't2'], bounds={'t1': bounds[0], 't2': bounds[1]})
    m.update(X, y)
    pri = G.default_priors(bounds, y)
    h0 = G.initial_hyper(y)
    assert m._hyper == h0
    m.optimize()
    info = m._opt_info
    href, iref = HO.optimize(X, y, h0, pri, max_iters=50)
    fg, fc = np.array(info['objective']), np.array(iref['objective'])
    assert len(fg) == len(fc), (len(fg), len(fc), info['status'], iref['status'])
    assert info['n_fits'] == iref['n_fits']
    scale = abs(fc[0] - fc[-1]) + 1.0
    assert np.max(np.abs(fg - fc)) <= 5e-6 * scale, (np.max(np.abs(fg - fc)), scale)
    assert info['status'] == iref['status']
    # the end points: equally good under the ORACLE's objective (the search stops on a change of the objective, which
    # leaves the signal variance -- the flat direction at this size, measured 1e-3 relative -- only loosely determined)
    ref_obj = HO.MapObjective(X, y, pri)
    f_dev_end = ref_obj.value(H.logexp_inv(np.array([m._hyper[k] for k in H.NAMES])))
    f_ref_end = ref_obj.value(H.logexp_inv(np.array([href[k] for k in H.NAMES])))
    assert abs(f_dev_end - f_ref_end) <= 5e-6 * scale, (f_dev_end, f_ref_end, scale)
    for k in H.NAMES:
        assert abs(m._hyper[k] - href[k]) <= (5e-2 if k == 'bias' else 5e-3) * href[k], (k, m._hyper[k], href[k])
    assert fg[-1] < fg[0] - 1.0


def test_map_search_that_crosses_failed_plain_factorisations(hip_ctx):
    """A MAP search whose trial hyper-parameters make the PLAIN Cholesky fail (duplicate evidence points under a signal
    variance that swallows GPy's 1e-8; tests/test_gp_gpu.py: _jitter_problem) continues on jitchol's jittered factor, as
    the reference's does ([GPy-upstream] jitchol behind every objective evaluation of GPyRegression.optimize,
    gpy_regression.py:317-323) -- round 4's library stopped the search at the first such trial.  Device SCG next to the
    oracle's SCG from the same start: same number of iterations and rebuilds, same stopping reason, objective values per
    iteration within 1e-5 of the search's total decrease over the five iterations compared (every factor here belongs to a
    matrix of condition ~1e8, and SCG takes its curvature from gradient differences: the two implementations' trajectories
    separate by 1e-7 of the objective after three iterations, 1e-4 after six, 1e-1 after twelve -- measured)."""
    from elfi_amd import HipGPRegression
    rs = np.random.RandomState(3)
    n = 200
    X = rs.randint(-2, 3, (n, 2)).astype(float)
    X[0] = X[1] = 0.0
    y = (np.linalg.norm(X - 0.5, axis=1) + 0.1 * rs.randn(n))[:, None]
    bounds = [(-2, 2), (-2, 2)]
    m = HipGPRegression(['a', 'b'], bounds={'a': bounds[0], 'b': bounds[1]}, max_opt_iters=5)
    m.update(X, y)
    pri = G.default_priors(bounds, y)
    h0 = dict(var=float(2 ** 30), ls=1.0, bias=1e-3, noise=1e-12)
    m._hyper = dict(h0)
    m._refit()
    assert m._handle.jitchol()[1] == 1                   # the start itself needs the ladder
    m.optimize()
    info = m._opt_info
    href, iref = HO.optimize(X, y, h0, pri, max_iters=5)
    fg, fc = np.array(info['objective']), np.array(iref['objective'])
    assert len(fg) == len(fc) and info['n_fits'] == iref['n_fits'], (len(fg), len(fc), info['n_fits'], iref['n_fits'])
    assert info['status'] == iref['status']
    scale = abs(fc[0] - fc[-1]) + 1.0
    assert np.max(np.abs(fg - fc)) <= 1e-5 * scale, (np.max(np.abs(fg - fc)), scale)
    assert fg[-1] < fg[0] - 1.0
    for k in ('var', 'ls', 'bias', 'noise'):
        assert abs(m._hyper[k] - href[k]) <= 1e-2 * abs(href[k]) + 1e-14, (k, m._hyper[k], href[k])


def test_whole_scg_search_at_d_10_next_to_the_oracle(hip_ctx):
    """A second shape for row a10 (the published pin is one d = 2 run): ONE whole MAP search in TEN dimensions -- the
    BASELINE first-metric surrogate (X uniform in [-2, 2]^10, y = |x - 0.5| + noise, SURVEY.md 8d "G-1") at n = 768 -- on
    the device next to the oracle's SCG from the reference's start (GPy's kernel defaults, noise max(y)^2 / 100): same
    iterations, evaluations and stopping reason, per-iteration objectives within 5e-6 of the total decrease, end points
    equally good under the oracle's objective."""
    from elfi_amd import HipGPRegression
    from elfi_amd import hyperopt as H
    n, d = 768, 10
    rs = np.random.RandomState(10)
    X = rs.uniform(-2, 2, (n, d))
    y = (np.linalg.norm(X - 0.5, axis=1) + 0.1 * rs.randn(n))[:, None]
    names = ['p%d' % i for i in range(d)]
    bounds = [(-2, 2)] * d
    m = HipGPRegression(names, bounds=dict(zip(names, bounds)))
    m.update(X, y)
    pri = G.default_priors(bounds, y)
    h0 = G.initial_hyper(y)
    assert m.hyperparameters == h0
    m.optimize()
    info = m._opt_info
    href, iref = HO.optimize(X, y, h0, pri, max_iters=50)
    fg, fc = np.array(info['objective']), np.array(iref['objective'])
    assert len(fg) == len(fc), (len(fg), len(fc), info['status'], iref['status'])
    assert info['n_fits'] == iref['n_fits'] and info['status'] == iref['status']
    scale = abs(fc[0] - fc[-1]) + 1.0
    assert np.max(np.abs(fg - fc)) <= 5e-6 * scale, (np.max(np.abs(fg - fc)), scale)
    ref_obj = HO.MapObjective(X, y, pri)
    f_dev_end = ref_obj.value(H.logexp_inv(np.array([m.hyperparameters[k] for k in H.NAMES])))
    f_ref_end = ref_obj.value(H.logexp_inv(np.array([href[k] for k in H.NAMES])))
    assert abs(f_dev_end - f_ref_end) <= 5e-6 * scale, (f_dev_end, f_ref_end, scale)
    for k in H.NAMES:
        assert abs(m.hyperparameters[k] - href[k]) <= (5e-2 if k == 'bias' else 5e-3) * href[k], (k, m.hyperparameters[k], href[k])
    assert fg[-1] < fg[0] - 1.0
