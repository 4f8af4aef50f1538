"""No GPU: the NumPy statement of the search for the GP mean's minimiser (tests/de_ref.py) against the fixture
tests/golden/demin.npz (scripts/make_golden_demin.py), and the host side of the device search.

  * the statement ends, on every fixture case, within the location bound the device search is held to
    (tests/test_gp_minimize_gpu.py): |x - x*|_inf <= max(16 e_ref, 2e-5), e_ref the reference's own distance from the
    refined minimiser x*;
  * its start population is a latin hypercube; the Philox counters of different (generation, member, slot) never coincide;
  * `elfi_amd.stochastic_optimization` hands any callable that is not a device model's `predict_mean` to the reference's own
    function; argument errors are raised before any device call.
"""
import os
import sys

import numpy as np
import pytest

import de_ref as D
from conftest import GOLDEN

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
sys.path.insert(0, ORACLE)
import ref_shim  # noqa: E402
import gp_oracle as G  # noqa: E402

N_CASES = 6


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLDEN, 'demin.npz'))


def case_of(gold, ci):
    keys = ('X', 'y', 'hyper', 'bounds', 'x_ref', 'x_star', 'e_ref', 'excess_ref')
    return {k: gold['%s_%d' % (k, ci)] for k in keys}


def location_bound(e_ref):
    return max(16.0 * float(e_ref), 2e-5)


def cpu_mean(c):
    post = G.Posterior(c['X'], c['y'], *c['hyper'], need_inv=False)
    return D.GPMean(c['X'], post.alpha, *c['hyper'][:3])


def test_fixture_matches_the_recipe(gold):
    assert [tuple(r) for r in gold['cases']] == [(3, 1, 0), (255, 2, 0), (257, 2, 0), (300, 5, 0), (600, 25, 0), (200, 2, 1)]
    for ci in range(N_CASES):
        c = case_of(gold, ci)
        n, d, edge = gold['cases'][ci]
        assert c['X'].shape == (n, d) and c['bounds'].shape == (d, 2)
        on_edge = c['x_star'] == c['bounds'][:, 1]
        assert on_edge[0] if edge else not on_edge.any()
        assert gold['pin_gap_%d' % ci] > 0
    assert gold['pin_gap_%d' % int(gold['pin_case'])] > 1e-9


@pytest.mark.parametrize('ci', range(N_CASES))
def test_statement_ends_within_the_location_bound(gold, ci):
    c = case_of(gold, ci)
    mean = cpu_mean(c)
    res = D.minimize(mean, c['bounds'][:, 0], c['bounds'][:, 1], seed=int(gold['ref_seed']))
    dist = float(np.max(np.abs(res['x'] - c['x_star'])))
    print('case %d: e_ref %.3e, statement %.3e after %d generations' % (ci, c['e_ref'], dist, res['generations']))
    assert res['converged'] and dist <= location_bound(c['e_ref'])
    if gold['cases'][ci][2]:
        assert res['x'][0] == c['bounds'][0, 1]


@pytest.mark.parametrize('d,NP', [(1, 5), (2, 30), (5, 75), (25, 375)])
def test_start_population_is_a_latin_hypercube(d, NP):
    pop = D.start_population(d, NP, seed=3)
    assert pop.shape == (NP, d) and np.all((pop >= 0) & (pop < 1))
    strata = np.floor(pop * NP).astype(int)
    for j in range(d):
        assert np.array_equal(np.sort(strata[:, j]), np.arange(NP))
    assert not np.array_equal(pop, D.start_population(d, NP, seed=4))


@pytest.mark.parametrize('d', [1, 2, 25, 256])
def test_counters_of_different_draws_never_coincide(d):
    NP = max(5, 15 * d)
    i, s = np.meshgrid(np.arange(NP), np.arange(D.n_slots(d)), indexing='ij')
    low = D.counter(0, i, s, d)
    assert np.unique(low).size == NP * D.n_slots(d) and int(low.max()) < 2 ** 32
    # the generation is the counter's high word: two generations share no counter whatever member and slot
    for g in (1, 2, 1000, 2 ** 31):
        c = D.counter(g, i, s, d)
        assert np.array_equal(c >> np.uint64(32), np.full(c.shape, g, dtype=np.uint64))
        assert np.array_equal(c & np.uint64(0xffffffff), low)


def test_trial_indices_are_distinct(gold):
    pop = D.start_population(2, 30, seed=5)
    E = np.arange(30.0)[::-1].copy()
    for g in range(1, 40):
        T, parts = D.trials(pop, E, g, seed=5)
        i = np.arange(30)
        assert np.all(parts['r0'] != i) and np.all(parts['r1'] != i) and np.all(parts['r0'] != parts['r1'])
        assert np.all((parts['r0'] >= 0) & (parts['r0'] < 30) & (parts['r1'] >= 0) & (parts['r1'] < 30))
        assert 0.5 <= parts['F'] < 1.0 and np.all((T >= 0) & (T <= 1))


@pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')
def test_host_callable_goes_to_the_reference_function():
    ref_shim.install()
    import elfi_amd
    from elfi.methods.bo.utils import stochastic_optimization

    def fun(x):
        x = np.atleast_2d(x)
        return ((x - np.array([0.3, -0.2])) ** 2).sum(axis=1, keepdims=True) + np.cos(3 * x[:, :1])

    bounds = [(-2, 2), (-1, 1)]
    x, f = elfi_amd.stochastic_optimization(fun, bounds, maxiter=50, polish=True, seed=3)
    xr, fr = stochastic_optimization(fun, bounds, maxiter=50, polish=True, seed=3)
    assert np.array_equal(x, xr) and f == fr
    # an unfitted device model's predict_mean is a host callable like any other (zeros: the reference's behaviour)
    gp = elfi_amd.HipGPRegression(['a', 'b'], bounds={'a': (-2, 2), 'b': (-1, 1)})
    x, f = elfi_amd.stochastic_optimization(gp.predict_mean, gp.bounds, maxiter=2, seed=3)
    xr, fr = stochastic_optimization(gp.predict_mean, gp.bounds, maxiter=2, seed=3)
    assert np.array_equal(x, xr) and f == fr


def test_argument_errors_come_before_any_device_call():
    import elfi_amd
    from elfi_amd.gp import check_minimize_arguments
    lo, hi = check_minimize_arguments(2, [(-2, 2), (-1, 1)])
    assert np.array_equal(lo, [-2, -1]) and np.array_equal(hi, [2, 1])
    with pytest.raises(ValueError, match='one .lower, upper. pair per input dimension'):
        check_minimize_arguments(2, [(-2, 2)])
    with pytest.raises(ValueError, match='one .lower, upper. pair per input dimension'):
        check_minimize_arguments(1, [(-2, 2), (0, 1)])
    with pytest.raises(ValueError, match='lower < upper'):
        check_minimize_arguments(2, [(-2, 2), (1, 1)])
    with pytest.raises(ValueError, match='lower < upper'):
        check_minimize_arguments(2, [(-2, np.inf), (0, 1)])
    with pytest.raises(ValueError, match='popsize'):
        check_minimize_arguments(2, [(-2, 2), (0, 1)], popsize=0)
    with pytest.raises(ValueError, match='population limit'):
        check_minimize_arguments(256, [(0, 1)] * 256, popsize=16)
    with pytest.raises(ValueError, match='maxiter'):
        check_minimize_arguments(2, [(-2, 2), (0, 1)], maxiter=-1)
    with pytest.raises(ValueError, match='tol'):
        check_minimize_arguments(2, [(-2, 2), (0, 1)], tol=-0.1)
    # through the model: nothing below has a device object to call
    bad = elfi_amd.HipGPRegression(['a', 'b'], bounds={'a': (1, 0), 'b': (0, 1)})
    with pytest.raises(ValueError, match='lower < upper'):
        bad.minimize_mean()
    gp = elfi_amd.HipGPRegression(['a', 'b'], bounds={'a': (-2, 2), 'b': (-1, 1)})
    assert gp._handle is None
    with pytest.raises(ValueError, match='popsize'):
        gp.minimize_mean(popsize=0)
    with pytest.raises(RuntimeError, match='no evidence yet'):
        gp.minimize_mean()
    assert gp._handle is None
