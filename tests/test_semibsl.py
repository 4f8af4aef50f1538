"""CPU: the NumPy/SciPy statement of the semiparametric synthetic likelihood (tests/semibsl_ref.py) against the values
recorded from the reference's own function (tests/golden/semibsl.npz, scripts/make_golden_semibsl.py), and the argument
handling of the Python mirrors (elfi_amd/synlik.py), which happens before any device call.

Tolerance: the yardstick is `truth` (the quantity in 60-digit arithmetic).  A value must lie within
16 x max(e_ref over the recorded cases with the same number of summaries m, tied twins included),
e_ref = |reference - truth| -- the rule of tests/test_synlik.py.
"""
import os
from functools import partial

import numpy as np
import pytest

import semibsl_ref as R


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'semibsl.npz'))


def bound_for(gold, m):
    """16 x the largest recorded error of the reference over every case (plain and tied) with m summaries."""
    e = [gold['e_ref'][i].max() for i, c in enumerate(R.CASES) if c[2] == m]
    if m == 2:      # the MA2 likelihoods (two summaries) are recorded cases of m = 2 as well
        e.append(np.abs((gold['sl_ref'] - gold['sl_truth_hi']) - gold['sl_truth_lo']).max())
        e.append(np.abs((gold['pen_ref'] - gold['pen_truth_hi']) - gold['pen_truth_lo']).max())
    return 16.0 * max(e)


def test_fixture_matches_the_recipe(gold):
    assert np.array_equal(gold['cases'], np.array(R.CASES, dtype=float))
    assert gold['ref'].shape == (len(R.CASES), 2, len(R.CONFIGS))
    assert [(c[1], c[2]) for c in R.CASES] == [(5, 1), (100, 2), (33, 15), (40, 16), (257, 17), (500, 8), (255, 33),
                                               (300, 64), (1000, 32)]
    assert np.all(np.isfinite(gold['ref'])) and np.all(gold['e_ref'] < 1e-9)
    X, y = R.make_case(*R.TWO_VALUED[:1], tied=True)
    assert len(np.unique(X[:, R.TWO_VALUED[1]])) == 2
    for n in R.SCORE_TABLES:
        assert gold['ppf_%d_hi' % n].shape == (n,) and (n % 2 == 0 or gold['ppf_%d_hi' % n][n // 2] == 0.0)


@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_restatement_against_truth_and_reference(gold, ci):
    case = R.CASES[ci]
    tol = bound_for(gold, case[2])
    for ti in (0, 1):
        X, y = R.make_case(ci, tied=bool(ti))
        for ki, name in enumerate(R.CONFIGS):
            got = R.semi_loglik_ref(X, y, **R.config_kwargs(name))[0, 0, 0]
            dev = abs((got - gold['truth_hi'][ci, ti, ki]) - gold['truth_lo'][ci, ti, ki])
            print('n=%d m=%d %s %-8s e_ref %.2e restatement %.2e bound %.2e'
                  % (case[1], case[2], 'tied ' if ti else 'plain', name, gold['e_ref'][ci, ti, ki], dev, tol))
            assert dev <= tol, (name, ti, dev, tol)
            assert abs(got - gold['ref'][ci, ti, ki]) <= tol + gold['e_ref'][ci, ti, ki]


def test_restatement_prefixes_penalties_groups_and_degenerate_cases():
    X, y = R.make_case(5)
    n = len(X)
    full = R.semi_loglik_ref(X, y, prefixes=[100, 250, n], shrinkage='warton', penalties=R.PENALTIES)
    assert full.shape == (1, 3, 3)
    for k, p in enumerate([100, 250, n]):
        for j, pen in enumerate(R.PENALTIES):
            assert full[0, k, j] == R.semi_loglik_ref(X[:p], y, shrinkage='warton', penalty=pen)[0, 0, 0]
    two = R.semi_loglik_ref(X, y, n_groups=2)
    assert two[0, 0, 0] == R.semi_loglik_ref(X[:250], y)[0, 0, 0] and two[1, 0, 0] == R.semi_loglik_ref(X[250:], y)[0, 0, 0]
    assert np.array_equal(R.ranks([3.0, 1.0, 3.0, 2.0]), [3.5, 1.0, 3.5, 2.0])
    far = y.copy()
    far[0] += 60 * X[:, 0].std()
    assert R.semi_loglik_ref(X, far)[0, 0, 0] == -np.inf
    const = X.copy()
    const[:, 2] = 1.0
    assert R.semi_loglik_ref(const, y)[0, 0, 0] == -np.inf
    assert R.semi_loglik_ref(X[:2], y)[0, 0, 0] == -np.inf


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib, synlik

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    rs = np.random.RandomState(0)
    X, y = rs.randn(40, 3), rs.randn(3)
    with pytest.raises(NotImplementedError):
        elfi_amd.semi_loglik(X, y, shrinkage='glasso', penalty=0.1)
    with pytest.raises(NotImplementedError):
        elfi_amd.semiparametric_likelihood(shrinkage='glasso', penalty=0.1)
    with pytest.raises(NotImplementedError):
        elfi_amd.semiparametric_likelihood(whitening=np.eye(3))
    with pytest.raises(NotImplementedError):
        elfi_amd.semiparametric_likelihood()(X, y, whitening=np.eye(3))
    with pytest.raises(NotImplementedError):
        elfi_amd.select_penalty(None, 100, [0.6, 0.2], ['S1'], likelihood=elfi_amd.semiparametric_likelihood(),
                                whitening=np.eye(3))
    with pytest.raises(NotImplementedError):
        elfi_amd.select_penalty(None, 100, [0.6, 0.2], ['S1'], likelihood=elfi_amd.semiparametric_likelihood(),
                                shrinkage='glasso')
    for kw in (dict(shrinkage='ridge', penalty=0.1), dict(shrinkage='warton'), dict(shrinkage='warton', penalty=1.5),
               dict(shrinkage='warton', penalties=[0.2, -0.1]), dict(penalties=[0.2]), dict(n_groups=3),
               dict(prefixes=[10, 10, 40]), dict(prefixes=[10, 30]), dict(prefixes=[1, 40]), dict(prefixes=[])):
        with pytest.raises(ValueError):
            elfi_amd.semi_loglik(X, y, **kw)
    with pytest.raises(TypeError):
        elfi_amd.semi_loglik(X, y, whitening=np.eye(3))             # the batched call has no such keyword
    with pytest.raises(ValueError):
        elfi_amd.semi_loglik(rs.randn(40, 65), rs.randn(65))
    with pytest.raises(ValueError):
        elfi_amd.semi_loglik(rs.randn(4, 3), y, n_groups=4)         # one row per group
    with pytest.raises(ValueError):
        elfi_amd.semi_loglik(np.zeros((synlik.MAX_SEMI_ROWS + 1, 1)), [0.0])
    with pytest.raises(ValueError):
        elfi_amd.semi_loglik(X, rs.randn(4))
    with pytest.raises(ValueError):
        elfi_amd.semiparametric_likelihood(shrinkage='ridge')
    with pytest.raises(TypeError):
        synlik._likelihood_setup(lambda ssx, ssy: 0.0)


def test_factories_have_the_reference_shapes():
    import elfi_amd
    from elfi_amd import synlik
    lik = elfi_amd.semiparametric_likelihood(shrinkage='warton', penalty=0.3)
    assert isinstance(lik, partial) and lik.func is synlik.semi_param_kernel_estimate
    assert lik.keywords == dict(shrinkage='warton', penalty=0.3, whitening=None)        # exactly the reference's keywords
    assert elfi_amd.semiparametric_likelihood().keywords == dict(shrinkage=None, penalty=None, whitening=None)
    assert 'adjustment' not in lik.keywords                                             # BSL must not take it for robust
    # the batched tools recognise the partial and send it to semi_loglik; the Gaussian default is untouched
    assert synlik._likelihood_setup(elfi_amd.semiparametric_likelihood()) == dict(semi=True, shrinkage=None, penalty=None)
    setup = synlik._likelihood_setup(lik, shrinkage='warton', whitening=None)
    assert setup == dict(semi=True, shrinkage='warton', penalty=0.3)
    assert synlik._likelihood_setup(None) == dict(shrinkage=None, penalty=None, whitening=None)
    assert synlik._likelihood_setup(synlik.semi_param_kernel_estimate) == dict(semi=True, shrinkage=None, penalty=None)
    assert elfi_amd.semi_loglik is synlik.semi_loglik
