"""GPU: the batched synthetic likelihood (csrc/synlik.hip through elfi_amd/synlik.py).

The yardstick of every log-likelihood is `truth` of tests/golden/synlik.npz (exact / 60-digit arithmetic on the same
float inputs), the bound 16 x max(e_ref over the recorded cases with the same m), e_ref = |reference - truth|
(tests/test_synlik.py: bound_for).  Quantities that are the same sums (prefixes, penalties, groups in one call against
single calls) must be equal bit for bit.

The reference for the MA2 tests is the copy oracle/make_ref.sh makes (oracle/ref_shim.py), as in
tests/test_reference_loop_gpu.py.

Measured on an MI355X (|device - truth| per case against e_ref): see DESIGN.md, "Bayesian synthetic likelihood".
"""
import os
import sys

import numpy as np
import pytest

import synlik_ref as R
from test_synlik import bound_for

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
sys.path.insert(0, ORACLE)
import ref_shim  # noqa: E402

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')

THETA, FEATS = [0.6, 0.2], ['S1', 'S2']


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'synlik.npz'))


@pytest.fixture(scope='module')
def elfi():
    e = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    return e


def _dev(got, hi, lo):
    return np.abs((np.asarray(got) - hi) - lo)


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_parity_with_truth_per_variant(hip_ctx, gold, ci):
    import elfi_amd
    case = R.CASES[ci]
    X, y, W, gamma = R.make_case(*case)
    tol = bound_for(gold, case[2])
    bad = []
    for ki, name in enumerate(R.CONFIGS):
        got = elfi_amd.syn_loglik(X, y, **R.config_kwargs(name, W, gamma))
        dev = _dev(got, gold['truth_hi'][ci, ki], gold['truth_lo'][ci, ki])
        print('n=%d m=%d %-9s device % .17g e_ref %.2e |device-truth| %.2e bound %.2e'
              % (case[1], case[2], name, got, gold['e_ref'][ci, ki], dev, tol))
        if not dev <= tol:
            bad.append((name, float(dev)))
    assert not bad, (bad, tol)


def test_callables_return_what_the_reference_returns(hip_ctx, gold):
    import elfi_amd
    X, y, W, gamma = R.make_case(*R.CASES[1])
    tol = bound_for(gold, 8)
    a = elfi_amd.standard_likelihood(shrinkage='warton', penalty=R.PENALTIES[1])(X, y[None, :])
    assert isinstance(a, np.ndarray) and a.shape == (1,)
    assert _dev(a[0], gold['truth_hi'][1, 6], gold['truth_lo'][1, 6]) <= tol
    b = elfi_amd.unbiased_likelihood()(X, y[None, :])
    assert isinstance(b, np.ndarray) and b.shape == (1,)
    assert _dev(b[0], gold['truth_hi'][1, 1], gold['truth_lo'][1, 1]) <= tol
    c = elfi_amd.robust_likelihood('mean')(X, y[None, :], gamma=gamma)
    assert np.ndim(c) == 0 and _dev(c, gold['truth_hi'][1, 2], gold['truth_lo'][1, 2]) <= tol
    ll, mean, cov = elfi_amd.syn_loglik(X, y, return_moments=True)
    np.testing.assert_allclose(mean[0], gold['mom_mean'], rtol=1e-13)
    np.testing.assert_allclose(cov[0], gold['mom_cov'], rtol=1e-11, atol=1e-11)
    assert np.array_equal(cov[0], cov[0].T)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci', [0, 1, 3, 4, 5])
def test_prefixes_and_penalties_in_one_call_equal_single_calls(hip_ctx, ci):
    import elfi_amd
    X, y, W, gamma = R.make_case(*R.CASES[ci])
    n, m = X.shape
    pre = sorted({max(m + 3, n // 7), n // 3 + 1, n // 3 + 2, n // 2, n - 5, n - 1, n})     # boundaries inside a 4-row step too
    for kw in (dict(), dict(whitening=W), dict(variant='unbiased')):
        one = elfi_amd.syn_loglik(X, y, prefixes=pre, **kw)
        for k, p in enumerate(pre):
            assert one[k] == elfi_amd.syn_loglik(X[:p], y, **kw), (kw.keys(), p)
    pens = [0.0, 0.1, 0.45, 1.0]
    both = elfi_amd.syn_loglik(X, y, prefixes=pre, shrinkage='warton', penalties=pens)
    assert both.shape == (len(pre), len(pens))
    for k, p in enumerate(pre):
        for j, pen in enumerate(pens):
            assert both[k, j] == elfi_amd.syn_loglik(X[:p], y, shrinkage='warton', penalty=pen), (p, pen)


# 3 ---------------------------------------------------------------------------------------------------------------
def test_64_groups_in_one_call_equal_64_single_calls(hip_ctx):
    import elfi_amd
    rs = np.random.RandomState(21)
    G, n, m = 64, 500, 20
    loc = rs.uniform(-30, 30, m)
    X = rs.randn(G, n, m) * np.linspace(1, 10, m) + loc
    y = loc + 0.5 * np.linspace(1, 10, m) * rs.randn(m)     # near the centre: psi of the unbiased estimator stays positive definite
    for kw in (dict(), dict(shrinkage='warton', penalty=0.3), dict(variant='unbiased')):
        all_, mean, cov = elfi_amd.syn_loglik(X, y, return_moments=True, **kw)
        assert all_.shape == (G,) and np.all(np.isfinite(all_))
        for g in range(G):
            ll, mg, cg = elfi_amd.syn_loglik(X[g], y, return_moments=True, **kw)
            assert ll == all_[g] and np.array_equal(mg[0], mean[g]) and np.array_equal(cg[0], cov[g])
    flat = elfi_amd.syn_loglik(X.reshape(G * n, m), y, n_groups=G)
    assert np.array_equal(flat, elfi_amd.syn_loglik(X, y))


def test_device_pointer_form_and_pitched_rows_equal_the_host_form(hip_ctx):
    """elfihip_syn_loglik_dev on torch tensors, rows with a pitch wider than m, and the host form with such a pitch:
    the same bits as the contiguous host call."""
    import torch
    import elfi_amd
    from elfi_amd import _lib
    X, y, W, gamma = R.make_case(*R.CASES[5])
    n, m = X.shape
    G, ng, ldx = 2, n // 2, m + 5
    pre = np.array([ng // 2 + 1, ng], dtype=np.int64)
    pens = np.array([0.1, 0.6])
    for code, kw in ((0, dict(shrinkage='warton', penalties=list(pens), whitening=W)), (3, dict(adjustment='variance', gamma=gamma))):
        want, wmean, wcov = elfi_amd.syn_loglik(X, y, n_groups=G, prefixes=pre, return_moments=True, **kw)
        want = want.reshape(G, len(pre), -1)
        P = want.shape[2] if code == 0 else 0
        wide = np.full((n, ldx), np.nan)
        wide[:, :m] = X
        # host form, pitched
        ll, mean, cov = np.empty_like(want), np.empty((G, m)), np.empty((G, m, m))
        hip_ctx.call("elfihip_syn_loglik", _lib.ptr(wide), G, ng, m, ldx, _lib.ptr(y), _lib.ptr(W) if code == 0 else None,
                     code, _lib.ptr(gamma) if code else None, _lib.ptr(pre), len(pre), _lib.ptr(pens) if P else None, P,
                     _lib.ptr(ll), _lib.ptr(mean), _lib.ptr(cov))
        assert np.array_equal(ll, want) and np.array_equal(mean, wmean) and np.array_equal(cov, wcov)
        # device form, pitched
        dev = torch.device('cuda')
        dX, dy = torch.from_numpy(wide).to(dev), torch.from_numpy(y).to(dev)
        dW, dg = torch.from_numpy(W).to(dev), torch.from_numpy(gamma).to(dev)
        dll = torch.zeros(want.shape, dtype=torch.float64, device=dev)
        dmean = torch.zeros((G, m), dtype=torch.float64, device=dev)
        dcov = torch.zeros((G, m, m), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        hip_ctx.call("elfihip_syn_loglik_dev", dX.data_ptr(), G, ng, m, ldx, dy.data_ptr(), dW.data_ptr() if code == 0 else None,
                     code, dg.data_ptr() if code else None, _lib.ptr(pre), len(pre), _lib.ptr(pens) if P else None, P,
                     dll.data_ptr(), dmean.data_ptr(), dcov.data_ptr())
        hip_ctx.synchronize()
        assert np.array_equal(dll.cpu().numpy(), want)
        assert np.array_equal(dmean.cpu().numpy(), wmean) and np.array_equal(dcov.cpu().numpy(), wcov)


def test_c_entry_point_refuses_bad_arguments(hip_ctx):
    """ELFIHIP_ERR_ARG before any launch: the output keeps its sentinel.  The lists are refused in the words
    elfihip_semi_loglik uses for the same lists (one check serves both: csrc/group_args.hpp)."""
    from elfi_amd import _lib
    SENTINEL = -12345.5
    X, y, gam = np.zeros((8, 3)), np.zeros(3), np.zeros(3)
    ll = np.full(4, SENTINEL)
    pre, pens = np.array([4, 8], dtype=np.int64), np.array([0.5, 1.5])

    def call(G=1, n=8, m=3, ldx=3, variant=0, gamma=None, pre=None, K=0, pens=None, P=0):
        hip_ctx.call("elfihip_syn_loglik", _lib.ptr(X), G, n, m, ldx, _lib.ptr(y), None, variant, _lib.ptr(gamma),
                     _lib.ptr(pre), K, _lib.ptr(pens), P, _lib.ptr(ll), None, None)

    def semi_text(pre=None, K=0, pens=None, P=0):
        with pytest.raises(ValueError) as exc:
            hip_ctx.call("elfihip_semi_loglik", _lib.ptr(X), 1, 8, 3, 3, _lib.ptr(y), _lib.ptr(pre), K, _lib.ptr(pens), P,
                         _lib.ptr(ll), None, None, None)
        return str(exc.value)

    reversed_pre, bad_pens = dict(pre=pre[::-1].copy(), K=2), dict(pens=pens, P=2)
    for kw in (dict(m=65), dict(n=1), dict(ldx=2), dict(G=0), dict(variant=4), dict(variant=2), reversed_pre,
               dict(pre=pre[:1].copy(), K=1), dict(pre=np.array([1, 8], dtype=np.int64), K=2), bad_pens,
               dict(variant=1, pens=np.array([0.5]), P=1)):
        with pytest.raises(ValueError) as exc:
            call(**kw)
        assert np.all(ll == SENTINEL), kw
        if kw is reversed_pre or kw is bad_pens:
            assert str(exc.value) == semi_text(**kw)
            assert np.all(ll == SENTINEL), kw
    assert semi_text(**reversed_pre) == 'prefixes must be ascending and at least 2 (entry 1)'
    assert semi_text(**bad_pens) == 'penalty 1 is outside [0, 1]'
    call(variant=2, gamma=gam, pre=pre, K=2)     # the call itself is sound: good arguments go through
    assert not np.any(ll[:2] == SENTINEL) and np.all(ll[2:] == SENTINEL)


# 4---------------------------------------------------------------------------------------------------------------
def test_singular_and_non_finite_groups_give_minus_infinity(hip_ctx):
    import elfi_amd
    X, y, W, gamma = R.make_case(*R.CASES[1])
    rep = np.tile(X[:1], (200, 1))                       # one row repeated: the covariance is the zero matrix
    for kw in (dict(), dict(variant='unbiased'), dict(adjustment='mean', gamma=gamma)):
        assert elfi_amd.syn_loglik(rep, y, **kw) == -np.inf
    three = np.stack([X[:200], rep, X[200:400]])         # the groups beside it are not disturbed
    got = elfi_amd.syn_loglik(three, y)
    assert got[1] == -np.inf and got[0] == elfi_amd.syn_loglik(X[:200], y) and got[2] == elfi_amd.syn_loglik(X[200:400], y)
    for bad in (np.nan, np.inf, -np.inf):
        Z = X[:200].copy()
        Z[150, 3] = bad
        pre = elfi_amd.syn_loglik(Z, y, prefixes=[100, 200])
        assert pre[1] == -np.inf and pre[0] == elfi_amd.syn_loglik(X[:100], y)   # the prefix in front of it is whole
    # psi of the unbiased estimator is not positive definite when y is far out
    assert elfi_amd.syn_loglik(X[:50], y + 1e3, variant='unbiased') == -np.inf


# 5 ---------------------------------------------------------------------------------------------------------------
def _ma2_matrices(model, max_sim, M, seed):
    """The matrices log_SL_stdev / select_penalty draw: child seed i of SeedSequence(seed) -> one generate call."""
    at = {name: value for name, value in zip(model.parameter_names, THETA)}
    y = np.array([np.ravel(model[f].observed)[0] for f in FEATS])
    mats = np.empty((M, max_sim, len(FEATS)))
    for i, child in enumerate(np.random.SeedSequence(seed).generate_state(M)):
        sims = model.generate(max_sim, outputs=FEATS, with_values=at, seed=child)
        for c, f in enumerate(FEATS):
            mats[i, :, c] = np.ravel(sims[f])
    return mats, y


@needs_reference
def test_log_SL_stdev_and_select_penalty_reproduce_the_reference(hip_ctx, elfi, gold):
    import elfi_amd
    from elfi.examples import ma2
    model = ma2.get_model(seed_obs=4)
    tol = bound_for(gold, 2)
    # every likelihood the two tools evaluate, against truth
    mats, obs = _ma2_matrices(model, int(gold['sl_n_sim'].max()), int(gold['sl_M']), int(gold['sl_seed']))
    ll = elfi_amd.syn_loglik(mats, obs, prefixes=gold['sl_n_sim'])
    dev = _dev(ll, gold['sl_truth_hi'], gold['sl_truth_lo']).max()
    print('log_SL_stdev likelihoods: max |device-truth| %.2e bound %.2e' % (dev, tol))
    assert dev <= tol
    mats, obs = _ma2_matrices(model, int(gold['pen_n_sim'].max()), int(gold['pen_M']), int(gold['pen_seed']))
    lmdas = list(np.arange(0.2, 0.8, 0.02))
    ll = elfi_amd.syn_loglik(mats, obs, prefixes=gold['pen_n_sim'], shrinkage='warton', penalties=lmdas)
    dev = _dev(ll, gold['pen_truth_hi'], gold['pen_truth_lo']).max()
    print('select_penalty likelihoods: max |device-truth| %.2e bound %.2e' % (dev, tol))
    assert dev <= tol
    # the tools themselves: a standard deviation moves by no more than the largest change of a likelihood, which is at
    # most |device - truth| + |reference - truth| <= tol + tol / 16
    std = elfi_amd.log_SL_stdev(model, THETA, list(gold['sl_n_sim']), FEATS, M=int(gold['sl_M']), seed=int(gold['sl_seed']))
    assert std.shape == gold['sl_std'].shape and np.abs(std - gold['sl_std']).max() <= tol * 17 / 16
    # simulation counts in any order, repeated ones too
    std2 = elfi_amd.log_SL_stdev(model, THETA, [200, 50, 50], FEATS, M=int(gold['sl_M']), seed=int(gold['sl_seed']))
    assert np.array_equal(std2, std[[2, 0, 0]])
    lm, sd = elfi_amd.select_penalty(model, list(gold['pen_n_sim']), THETA, FEATS, M=int(gold['pen_M']),
                                     shrinkage='warton', seed=int(gold['pen_seed']))
    assert np.array_equal(lm, gold['pen_lmdas'])
    assert np.abs(sd - gold['pen_stds']).max() <= tol * 17 / 16


# 6 ---------------------------------------------------------------------------------------------------------------
def _check_chain(bsl, gold, tol):
    params, logpost = bsl.state['params'], bsl.state['logposterior']
    moved = np.any(np.diff(params, axis=0) != 0, axis=1)
    ref_moved = np.any(np.diff(gold['bsl_params'], axis=0) != 0, axis=1)
    flips = np.flatnonzero(moved != ref_moved)
    assert flips.size == 0, 'accept/reject differs from the reference first at sample %d (reference logposterior %r, ' \
        'device %r)' % (flips[0] + 1, gold['bsl_logpost'][flips[0] + 1], logpost[flips[0] + 1])
    assert np.abs(params - gold['bsl_params']).max() <= tol * 17 / 16
    assert np.abs(logpost - gold['bsl_logpost']).max() <= tol * 17 / 16


@needs_reference
def test_bsl_chain_reproduces_the_reference(hip_ctx, elfi, gold):
    import elfi_amd
    from elfi.examples import ma2
    tol = bound_for(gold, 2)
    n, rnd, seed = int(gold['bsl_n']), int(gold['bsl_round']), int(gold['bsl_seed'])
    bsl = elfi.BSL(ma2.get_model(seed_obs=4), rnd, feature_names=FEATS, likelihood=elfi_amd.standard_likelihood(), seed=seed)
    res = bsl.sample(n, sigma_proposals=0.02 * np.eye(2), params0=THETA, bar=False)
    assert type(res).__name__ == 'BslSample'
    _check_chain(bsl, gold, tol)
    hip = elfi_amd.HipBSL(ma2.get_model(seed_obs=4), rnd, feature_names=FEATS, seed=seed)
    assert isinstance(hip, elfi.BSL) and not hip.is_misspec
    hip.sample(n, sigma_proposals=0.02 * np.eye(2), params0=THETA, bar=False)
    _check_chain(hip, gold, tol)
    # the robust likelihood is recognised by BSL (bsl.py:54) and runs with the reference's gamma sampler
    rob = elfi_amd.HipBSL(ma2.get_model(seed_obs=4), rnd, feature_names=FEATS, likelihood=elfi_amd.robust_likelihood('mean'),
                          seed=seed)
    assert rob.is_misspec
    out = rob.sample(20, sigma_proposals=0.02 * np.eye(2), params0=THETA, bar=False)
    assert np.all(np.isfinite(rob.state['logposterior'])) and 'gamma' in out.samples_all
