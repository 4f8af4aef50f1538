"""CPU: the NumPy/SciPy statement of the whitened semiparametric synthetic likelihood (tests/wsemibsl_ref.py) against
`truth` of tests/golden/wsemibsl.npz (60-digit arithmetic; scripts/make_golden_wsemibsl.py), the condition on the inputs
that makes the truth the one answer, and the argument handling of elfi_amd/synlik.py, which comes before any device call.
Tolerance: 16 x the largest of max(e_ref, e_np) over the recorded cases with the same m, tied twins included;
e_ref = |reference - truth|, e_np = |NumPy statement - truth|, both recorded in the fixture."""
import os
from functools import partial

import numpy as np
import pytest

import wsemibsl_ref as R


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'wsemibsl.npz'))


def bound_for(gold, m, key=None):
    """16 x the largest recorded error over every case with m summaries: of the likelihood, or of a stage (`key`)."""
    rows = [vi for vi, (ci, _) in enumerate(R.variants()) if R.S.CASES[ci][2] == m]
    if key is not None:
        return 16.0 * gold[key][rows].max()
    return 16.0 * max(np.nanmax(gold['e_ref'][rows], initial=0.0), gold['e_np'][rows].max())


def test_fixture_matches_the_recipe_and_the_gap_condition(gold):
    assert np.array_equal(gold['variants'], R.variants()) 
    assert [R.S.CASES[ci][1:3] for ci in R.CASES] == [(5, 1), (100, 2), (33, 15), (40, 16), (257, 17), (255, 33), (300, 64)]
    assert np.all(np.isfinite(gold['truth_hi'])) and np.all(gold['e_np'] < 1e-9)
    assert np.all(gold['gap'] >= R.MIN_GAP) and R.MIN_GAP == 1e-9


@pytest.mark.parametrize('vi', range(len(R.variants())))
def test_restatement_against_truth(gold, vi):
    ci, tied = R.variants()[vi]
    X, y, W = R.make_case(ci, tied)
    tol = bound_for(gold, X.shape[1])
    for ki, pen in enumerate(R.CONFIGS):
        kw = {} if pen is None else dict(shrinkage='warton', penalty=pen)
        got = R.wsemi_loglik_ref(X, y, W, **kw)
        dev = abs((got - gold['truth_hi'][vi, ki]) - gold['truth_lo'][vi, ki])
        assert dev <= tol, (pen, dev, tol)


def test_restatement_minus_infinity_rules():
    X, y, W = R.make_case(2)
    far = y.copy()
    far[0] += 60 * X[:, 0].std()
    assert R.wsemi_loglik_ref(X, far, W) == -np.inf
    const = X.copy()
    const[:, 2] = 1.0
    assert R.wsemi_loglik_ref(const, y, W) == -np.inf
    assert R.wsemi_loglik_ref(X[:2], y, W) == -np.inf
    Z = W.copy()
    Z[3] = 0.0                                                       # d_3 = 0
    assert R.wsemi_loglik_ref(X, y, Z) == -np.inf
    assert R.wsemi_loglik_ref(X, y, np.eye(15)) != R.S.semi_loglik_ref(X, y)[0, 0, 0]     # W = I is not semiBSL


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    rs = np.random.RandomState(0)
    X, y, W = rs.randn(40, 3), rs.randn(3), np.eye(3)
    for fn in (partial(elfi_amd.wsemi_loglik, X, y, W), partial(elfi_amd.whitened_semiparametric_likelihood, W)):
        with pytest.raises(NotImplementedError):
            fn(shrinkage='glasso', penalty=0.1)
    for bad in (np.eye(4), np.ones(3), None, np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            elfi_amd.wsemi_loglik(X, y, bad)
    for missing in (lambda: elfi_amd.wsemi_param_kernel_estimate(X, y), lambda: elfi_amd.whitened_semiparametric_likelihood(None)):
        with pytest.raises(ValueError):
            missing()
    for kw in (dict(shrinkage='warton'), dict(shrinkage='warton', penalty=1.5), dict(shrinkage='warton', penalties=[0.2, -0.1]),
               dict(penalties=[0.2]), dict(prefixes=[10, 10, 40]), dict(prefixes=[10, 30]), dict(prefixes=[1, 40])):
        with pytest.raises(ValueError):
            elfi_amd.wsemi_loglik(X, y, W, **kw)


def test_factory_and_routing():
    import elfi_amd
    from elfi_amd import synlik
    W = np.eye(3)
    lik = elfi_amd.whitened_semiparametric_likelihood(W, shrinkage='warton', penalty=0.3)
    assert isinstance(lik, partial) and lik.func is synlik.wsemi_param_kernel_estimate
    assert set(lik.keywords) == {'shrinkage', 'penalty', 'whitening'} and lik.keywords['whitening'] is W
    assert synlik._likelihood_setup(lik) == (synlik.wsemi_loglik, dict(shrinkage='warton', penalty=0.3, whitening=W))
    # select_penalty's call: its own whitening=None must not erase the partial's
    batched, setup = synlik._likelihood_setup(lik, shrinkage='warton', whitening=None)
    assert batched is synlik.wsemi_loglik and setup['whitening'] is W
    with pytest.raises(ValueError):
        synlik._likelihood_setup(synlik.wsemi_param_kernel_estimate)                    # the function alone has no W
    batched, setup = synlik._likelihood_setup(synlik.wsemi_param_kernel_estimate, whitening=W)
    assert batched is synlik.wsemi_loglik and setup['whitening'] is W
