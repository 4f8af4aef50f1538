"""CPU: the NumPy/SciPy statement of the synthetic likelihoods (tests/synlik_ref.py) against the values recorded from the
reference's own functions (tests/golden/synlik.npz, scripts/make_golden_synlik.py), and the argument handling of the
Python mirrors (elfi_amd/synlik.py), which happens before any device call.

Tolerance: the yardstick is `truth` (the quantity in exact / 60-digit arithmetic).  A value must lie within
16 x max(e_ref over the recorded cases with the same number of summaries m), e_ref = |reference - truth|.
"""
import os
from functools import partial

import numpy as np
import pytest

import synlik_ref as R


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'synlik.npz'))


def bound_for(gold, m):
    """16 x the largest recorded error of the reference over every case with m summaries."""
    e = [gold['e_ref'][i].max() for i, c in enumerate(R.CASES) if c[2] == m]
    if m == 2:      # the MA2 likelihoods (two summaries) are recorded cases of m = 2 as well
        e.append(np.abs((gold['sl_ref'] - gold['sl_truth_hi']) - gold['sl_truth_lo']).max())
        e.append(np.abs((gold['pen_ref'] - gold['pen_truth_hi']) - gold['pen_truth_lo']).max())
    return 16.0 * max(e)


def test_fixture_matches_the_recipe(gold):
    assert np.array_equal(gold['cases'], np.array(R.CASES, dtype=float))
    assert gold['ref'].shape == (len(R.CASES), len(R.CONFIGS))
    assert {(c[1], c[2]) for c in R.CASES} >= {(100, 2), (500, 8), (2000, 20), (5000, 32), (300, 64), (200, 40)}
    assert np.all(np.isfinite(gold['ref'])) and np.all(gold['e_ref'] < 1e-9)


@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_restatement_against_truth_and_reference(gold, ci):
    case = R.CASES[ci]
    X, y, W, gamma = R.make_case(*case)
    tol = bound_for(gold, case[2])
    for ki, name in enumerate(R.CONFIGS):
        got = R.syn_loglik_ref(X, y, **R.config_kwargs(name, W, gamma))[0, 0, 0]
        dev = abs((got - gold['truth_hi'][ci, ki]) - gold['truth_lo'][ci, ki])
        print('n=%d m=%d %-9s e_ref %.2e restatement %.2e bound %.2e' % (case[1], case[2], name, gold['e_ref'][ci, ki], dev, tol))
        assert dev <= tol, (name, dev, tol)
        assert abs(got - gold['ref'][ci, ki]) <= tol + gold['e_ref'][ci, ki]


def test_restatement_prefixes_penalties_groups_and_moments(gold):
    X, y, W, gamma = R.make_case(*R.CASES[1])
    n = len(X)
    full, mean, cov = R.syn_loglik_ref(X, y, prefixes=[100, 250, n], shrinkage='warton', penalties=R.PENALTIES,
                                       return_moments=True)
    assert full.shape == (1, 3, 3)
    for k, p in enumerate([100, 250, n]):
        for j, pen in enumerate(R.PENALTIES):
            assert full[0, k, j] == R.syn_loglik_ref(X[:p], y, shrinkage='warton', penalty=pen)[0, 0, 0]
    np.testing.assert_allclose(mean[0], gold['mom_mean'], rtol=1e-13)
    np.testing.assert_allclose(cov[0], gold['mom_cov'], rtol=1e-11, atol=1e-11)
    two = R.syn_loglik_ref(np.vstack([X[:250], X[250:]]), y, n_groups=2)
    assert two[0, 0, 0] == R.syn_loglik_ref(X[:250], y)[0, 0, 0] and two[1, 0, 0] == R.syn_loglik_ref(X[250:], y)[0, 0, 0]
    # a repeated row: no Cholesky factor
    assert R.syn_loglik_ref(np.tile(X[:1], (50, 1)), y)[0, 0, 0] == -np.inf


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib, synlik

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    rs = np.random.RandomState(0)
    X, y = rs.randn(40, 3), rs.randn(3)
    with pytest.raises(NotImplementedError):
        elfi_amd.syn_loglik(X, y, shrinkage='glasso', penalty=0.1)
    with pytest.raises(NotImplementedError):
        elfi_amd.standard_likelihood(shrinkage='glasso', penalty=0.1)
    with pytest.raises(NotImplementedError):
        elfi_amd.select_penalty(None, 100, [0.6, 0.2], ['S1'], shrinkage='glasso')
    for kw in (dict(shrinkage='ridge', penalty=0.1), dict(shrinkage='warton'), dict(shrinkage='warton', penalty=1.5),
               dict(shrinkage='warton', penalties=[0.2, -0.1]), dict(penalties=[0.2]), dict(n_groups=3),
               dict(variant='robust'), dict(adjustment='mean'), dict(adjustment='median', gamma=y), dict(variant='semi'),
               dict(prefixes=[10, 10, 40]), dict(shrinkage='warton', penalty=0.2, variant='unbiased'),
               dict(shrinkage='warton', penalty=0.2, adjustment='variance', gamma=y), dict(prefixes=[10, 30]), dict(prefixes=[1, 40]), dict(whitening=np.eye(2))):
        with pytest.raises(ValueError):
            elfi_amd.syn_loglik(X, y, **kw)
    with pytest.raises(ValueError):
        elfi_amd.syn_loglik(rs.randn(40, 65), rs.randn(65))
    with pytest.raises(ValueError):
        elfi_amd.syn_loglik(rs.randn(4, 3), y, n_groups=4)       # one row per group
    with pytest.raises(ValueError):
        elfi_amd.syn_loglik(X, rs.randn(4))
    with pytest.raises(ValueError):
        elfi_amd.robust_likelihood('median')
    with pytest.raises(TypeError):
        synlik._likelihood_setup(lambda ssx, ssy: 0.0)


def test_factories_have_the_reference_shapes():
    import elfi_amd
    from elfi_amd import synlik
    lik = elfi_amd.standard_likelihood(shrinkage='warton', penalty=0.3)
    assert isinstance(lik, partial) and lik.keywords == dict(shrinkage='warton', penalty=0.3, whitening=None)
    assert 'adjustment' not in lik.keywords
    rob = elfi_amd.robust_likelihood('variance')
    assert isinstance(rob, partial) and rob.keywords == {'adjustment': 'variance'}      # what BSL.__init__ looks for
    assert elfi_amd.unbiased_likelihood() is synlik.gaussian_syn_likelihood_ghurye_olkin
    assert synlik._likelihood_setup(None) == dict(shrinkage=None, penalty=None, whitening=None)
    assert synlik._likelihood_setup(lik, shrinkage='warton', whitening=None)['penalty'] == 0.3
    assert synlik._likelihood_setup(elfi_amd.unbiased_likelihood()) == dict(variant='unbiased')
    counts, uniq, where = synlik._prefix_axis([200, 50, 100, 50])
    assert list(uniq) == [50, 100, 200] and list(uniq[where]) == [200, 50, 100, 50]
