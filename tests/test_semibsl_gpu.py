"""GPU: the batched semiparametric synthetic likelihood (csrc/semibsl.hip through elfi_amd/synlik.py).

The yardstick of every log-likelihood is `truth` of tests/golden/semibsl.npz (60-digit arithmetic on the same float
inputs), the bound 16 x max(e_ref over the recorded cases with the same m, tied twins included),
e_ref = |reference - truth| (tests/test_semibsl.py: bound_for).  The stages are checked on their own through
return_parts, and quantities that are the same sums (prefixes, penalties, groups in one call against single calls, the
device-pointer form against the host form) must be equal bit for bit.

The normal scores are compared with a table of Phi^-1 at the exact rational i / (n + 1); the bound, 16 x the largest
relative error of SciPy's ndtri at the double i / (n + 1) over the same table, therefore contains the rounding of the
quotient, which the device and SciPy share (near p = 1/2 it dominates both).

No test calls the reference's semiparametric function (it does not run under this NumPy); the MA2 tests use the
reference's model, `model.generate` and `elfi.BSL` only (oracle/ref_shim.py), as tests/test_synlik_gpu.py does.

Measured on an MI355X (|device - truth| per case against e_ref): see DESIGN.md, "Semiparametric synthetic likelihood".
"""
import math
import os
import sys

import numpy as np
import pytest

import device_layout as DL
import semibsl_ref as R
from test_semibsl import bound_for

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
sys.path.insert(0, ORACLE)
import ref_shim  # noqa: E402

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')

THETA, FEATS = [0.6, 0.2], ['S1', 'S2']


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'semibsl.npz'))


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
def test_parity_with_truth(hip_ctx, gold, ci):
    import elfi_amd
    case = R.CASES[ci]
    tol = bound_for(gold, case[2])
    bad = []
    for ti in (0, 1):
        X, y = R.make_case(ci, tied=bool(ti))
        for ki, name in enumerate(R.CONFIGS):
            got = elfi_amd.semi_loglik(X, y, **R.config_kwargs(name))
            dev = _dev(got, gold['truth_hi'][ci, ti, ki], gold['truth_lo'][ci, ti, ki])
            print('n=%d m=%d %s %-8s device % .17g e_ref %.2e |device-truth| %.2e bound %.2e'
                  % (case[1], case[2], 'tied ' if ti else 'plain', name, got, gold['e_ref'][ci, ti, ki], dev, tol))
            if not dev <= tol:
                bad.append((name, ti, float(dev)))
    assert not bad, (bad, tol)


def test_callable_returns_an_array_of_one(hip_ctx, gold):
    import elfi_amd
    X, y = R.make_case(5)
    a = elfi_amd.semiparametric_likelihood(shrinkage='warton', penalty=R.PENALTIES[1])(X, y[None, :])
    assert isinstance(a, np.ndarray) and a.shape == (1,)
    assert _dev(a[0], gold['truth_hi'][5, 0, 2], gold['truth_lo'][5, 0, 2]) <= bound_for(gold, 8)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci', [0, 2, 4, 5, 8])
def test_stages(hip_ctx, gold, ci):
    import elfi_amd
    n, m = R.CASES[ci][1:3]
    for ti in (0, 1):
        X, y = R.make_case(ci, tied=bool(ti))
        ll, u, rho, scores = elfi_amd.semi_loglik(X, y, return_parts=True)
        assert u.shape == (1, m) and rho.shape == (1, m, m) and scores.shape == (1, n, m)
        u, rho, scores = u[0], rho[0], scores[0]
        ties = False
        for j in range(m):
            assert np.array_equal(np.argsort(scores[:, j], kind='stable'), np.argsort(X[:, j], kind='stable')), j
            vals, first, inv = np.unique(X[:, j], return_index=True, return_inverse=True)
            assert np.array_equal(scores[:, j], scores[first, j][inv]), j       # equal inputs, equal scores
            ties = ties or len(vals) < n
        if not ties:
            s0 = np.sort(scores[:, 0])
            for j in range(1, m):
                assert np.array_equal(np.sort(scores[:, j]), s0), j
            if n in R.SCORE_TABLES:
                hi, lo = gold['ppf_%d_hi' % n], gold['ppf_%d_lo' % n]
                yard = 16.0 * gold['ppf_%d_ndtri_rel' % n].max()
                nz = hi != 0.0
                rel = np.abs(((s0 - hi) - lo)[nz] / hi[nz]).max()
                print('n=%d scores: max relative error %.3e, ndtri %.3e, bound %.3e'
                      % (n, rel, gold['ppf_%d_ndtri_rel' % n].max(), yard))
                assert rel <= yard
                assert np.all(s0[~nz] == 0.0) and (n % 2 == 0 or s0[n // 2] == 0.0)     # Phi^-1(1/2) is exactly 0
        assert ti == 0 or ties
        assert np.array_equal(rho, rho.T) and np.all(np.diag(rho) == 1.0)
        err = np.abs(u - gold['u'][ci, ti, :m]).max()
        print('n=%d m=%d %s u: max |device-truth| %.2e' % (n, m, 'tied ' if ti else 'plain', err))
        assert err <= 1e-15


# 3 ---------------------------------------------------------------------------------------------------------------
def test_identities(hip_ctx):
    import elfi_amd
    # one column: the copula term is exactly zero, with any penalty
    X, y = R.make_case(0)
    one = elfi_amd.semi_loglik(X, y)
    assert np.isfinite(one)
    assert np.array_equal(elfi_amd.semi_loglik(X, y, shrinkage='warton', penalties=[0.0, 0.4, 1.0]), [one] * 3)
    for ci in (2, 5, 6):
        X, y = R.make_case(ci)
        m = X.shape[1]
        # penalty 1 leaves the KDE part alone: the sum of the one-column likelihoods, up to the order of that sum
        kde = math.fsum(elfi_amd.semi_loglik(X[:, [j]], y[[j]]) for j in range(m))
        got = elfi_amd.semi_loglik(X, y, shrinkage='warton', penalty=1.0)
        print('m=%d penalty 1: % .17g, sum of the columns % .17g' % (m, got, kde))
        assert abs(got - kde) <= m * 2.0 ** -50 * abs(kde)
        assert elfi_amd.semi_loglik(X, y, shrinkage='warton', penalties=[0.0])[0] == elfi_amd.semi_loglik(X, y)


# 4 ---------------------------------------------------------------------------------------------------------------
def test_minus_infinity_cases_leave_the_status_and_the_other_groups_alone(hip_ctx):
    import elfi_amd
    X, y = R.make_case(5)
    for sign, edge in ((1.0, 1.0), (-1.0, 0.0)):
        far = y.copy()
        far[0] += sign * 60 * X[:, 0].std()
        ll, u, rho, scores = elfi_amd.semi_loglik(X, far, return_parts=True)
        assert ll == -np.inf and u[0, 0] == edge and np.all((u[0, 1:] > 0) & (u[0, 1:] < 1))
    const = X[:200].copy()
    const[:, 2] = 1.0
    assert elfi_amd.semi_loglik(const, y) == -np.inf
    assert np.all(elfi_amd.semi_loglik(const, y, shrinkage='warton', penalties=[0.2, 1.0]) == -np.inf)
    assert elfi_amd.semi_loglik(X[:2], y) == -np.inf
    three = np.stack([X[:200], const, X[200:400]])
    got = elfi_amd.semi_loglik(three, y)
    assert got[1] == -np.inf and got[0] == elfi_amd.semi_loglik(X[:200], y) and got[2] == elfi_amd.semi_loglik(X[200:400], y)
    assert np.isfinite(got[0]) and np.isfinite(got[2])
    for bad in (np.nan, np.inf):
        Z = X[:200].copy()
        Z[150, 3] = bad
        pre = elfi_amd.semi_loglik(Z, y, prefixes=[100, 200])
        assert pre[1] == -np.inf and pre[0] == elfi_amd.semi_loglik(X[:100], y)   # the prefix in front of it is whole


# 5 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci,tied', [(2, False), (4, True), (5, False), (6, False)])
def test_prefixes_and_penalties_in_one_call_equal_single_calls(hip_ctx, ci, tied):
    import elfi_amd
    X, y = R.make_case(ci, tied=tied)
    n, m = X.shape
    pre = sorted(p for p in {max(m + 3, n // 7), 31, 32, 33, n // 2, n - 1, n} if 3 <= p <= n)
    one = elfi_amd.semi_loglik(X, y, prefixes=pre)
    for k, p in enumerate(pre):
        assert one[k] == elfi_amd.semi_loglik(X[:p], y), p
    pens = [0.0, 0.1, 0.45, 1.0]
    both = elfi_amd.semi_loglik(X, y, prefixes=pre, shrinkage='warton', penalties=pens)
    assert both.shape == (len(pre), len(pens))
    for k, p in enumerate(pre):
        for j, pen in enumerate(pens):
            assert both[k, j] == elfi_amd.semi_loglik(X[:p], y, shrinkage='warton', penalty=pen), (p, pen)


def test_64_groups_in_one_call_equal_64_single_calls(hip_ctx):
    import elfi_amd
    rs = np.random.RandomState(41)
    G, n, m = 64, 100, 8
    loc = rs.uniform(-30, 30, m)
    X = rs.randn(G, n, m) * np.linspace(1, 10, m) + loc
    y = loc + 0.5 * np.linspace(1, 10, m) * rs.randn(m)
    for kw in (dict(), dict(shrinkage='warton', penalty=0.3)):
        all_, u, rho, scores = elfi_amd.semi_loglik(X, y, return_parts=True, **kw)
        assert all_.shape == (G,) and np.all(np.isfinite(all_))
        for g in range(G):
            ll, ug, rg, sg = elfi_amd.semi_loglik(X[g], y, return_parts=True, **kw)
            assert ll == all_[g] and np.array_equal(ug[0], u[g]) and np.array_equal(rg[0], rho[g])
            assert np.array_equal(sg[0], scores[g])
    flat = elfi_amd.semi_loglik(X.reshape(G * n, m), y, n_groups=G)
    assert np.array_equal(flat, elfi_amd.semi_loglik(X, y))


def test_the_largest_group_and_the_raised_lds_limit(hip_ctx):
    """n = 16384 is the cap (one column and the reduction buffer fill 130 KB of LDS); from n = 5889 on the column kernel
    needs more dynamic LDS than the default limit.  Ranks, scores and the prefix rule at that size."""
    import elfi_amd
    rs = np.random.RandomState(43)
    n, m = 16384, 3
    X = rs.randn(2, n, m) * [1.0, 5.0, 0.1] + [0.0, 40.0, -3.0]
    X[1, :, 2] = np.round(X[1, :, 2] * 20) / 20                 # a tied column
    y = np.array([0.3, 41.0, -3.05])
    ll, u, rho, scores = elfi_amd.semi_loglik(X, y, prefixes=[5889, 8192, n], return_parts=True)
    assert ll.shape == (2, 3) and np.all(np.isfinite(ll)) and np.all((u > 0) & (u < 1))
    s0 = np.sort(scores[0, :, 0])
    assert np.all(np.diff(s0) > 0)
    for g, j in ((0, 1), (0, 2), (1, 0), (1, 1)):
        assert np.array_equal(np.sort(scores[g, :, j]), s0)
        assert np.array_equal(np.argsort(scores[g, :, j], kind='stable'), np.argsort(X[g, :, j], kind='stable'))
    vals, first, inv = np.unique(X[1, :, 2], return_index=True, return_inverse=True)
    assert len(vals) < n and np.array_equal(scores[1, :, 2], scores[1, first, 2][inv])
    assert np.array_equal(np.argsort(scores[1, :, 2], kind='stable'), np.argsort(X[1, :, 2], kind='stable'))
    for g in range(2):
        assert np.array_equal(rho[g], rho[g].T) and np.all(np.diag(rho[g]) == 1.0)
        for k, p in enumerate((5889, 8192)):
            assert ll[g, k] == elfi_amd.semi_loglik(X[g, :p], y), (g, p)
    with pytest.raises(ValueError):
        elfi_amd.semi_loglik(np.zeros((n + 1, 1)), [0.0])


def test_device_pointer_form_at_a_pitch_and_an_offset_equals_the_host_form(hip_ctx):
    """elfihip_semi_loglik_dev on torch tensors, rows at the pitch m + 3 from a base that is only 8-byte aligned, every
    output between sentinels; and the host form at that pitch: the same bits as the contiguous host call."""
    import elfi_amd
    from elfi_amd import _lib
    X, y = R.make_case(4)
    n, m = X.shape
    G, ng, ldx = 2, n // 2, m + 3
    X = X[:G * ng]
    pre = np.array([ng // 2 + 1, ng], dtype=np.int64)
    pens = np.array([0.1, 0.6])
    want, wu, wrho, wsc = elfi_amd.semi_loglik(X, y, n_groups=G, prefixes=pre, shrinkage='warton', penalties=list(pens),
                                               return_parts=True)
    assert want.shape == (G, 2, 2) and np.all(np.isfinite(want))
    wide = np.full((G * ng, ldx), np.nan)
    wide[:, :m] = X
    ll, u, rho, sc = np.empty_like(want), np.empty_like(wu), np.empty_like(wrho), np.empty_like(wsc)
    hip_ctx.call("elfihip_semi_loglik", _lib.ptr(wide), G, ng, m, ldx, _lib.ptr(y), _lib.ptr(pre), len(pre), _lib.ptr(pens),
                 len(pens), _lib.ptr(ll), _lib.ptr(u), _lib.ptr(rho), _lib.ptr(sc))
    assert np.array_equal(ll, want) and np.array_equal(u, wu) and np.array_equal(rho, wrho) and np.array_equal(sc, wsc)
    keep, dX = DL.place(X, ldx, 1)
    dy = DL.to_device(y)
    oll, ou = DL.guarded_out(G, 4, off=1), DL.guarded_out(G, m)
    orho, osc = DL.guarded_out(G, m * m, off=1), DL.guarded_out(G * ng, m)
    import torch
    torch.cuda.synchronize()
    hip_ctx.call("elfihip_semi_loglik_dev", dX, G, ng, m, ldx, dy.data_ptr(), _lib.ptr(pre), len(pre), _lib.ptr(pens),
                 len(pens), oll.ptr, ou.ptr, orho.ptr, osc.ptr)
    hip_ctx.synchronize()
    assert np.array_equal(oll.check().reshape(want.shape), want)
    assert np.array_equal(ou.check(), wu) and np.array_equal(orho.check().reshape(wrho.shape), wrho)
    assert np.array_equal(osc.check().reshape(wsc.shape), wsc)
    # the optional outputs left out
    oll2 = DL.guarded_out(G, 4)
    hip_ctx.call("elfihip_semi_loglik_dev", dX, G, ng, m, ldx, dy.data_ptr(), _lib.ptr(pre), len(pre), _lib.ptr(pens),
                 len(pens), oll2.ptr, None, None, None)
    hip_ctx.synchronize()
    assert np.array_equal(oll2.check().reshape(want.shape), want)


def test_c_entry_point_refuses_bad_arguments(hip_ctx):
    from elfi_amd import _lib
    X, y, ll = np.zeros((8, 3)), np.zeros(3), np.zeros(4)
    pre, pens = np.array([4, 8], dtype=np.int64), np.array([0.5, 1.5])

    def call(G=1, n=8, m=3, ldx=3, pre=None, K=0, pens=None, P=0):
        hip_ctx.call("elfihip_semi_loglik", _lib.ptr(X), G, n, m, ldx, _lib.ptr(y), _lib.ptr(pre), K, _lib.ptr(pens), P,
                     _lib.ptr(ll), None, None, None)
    for kw in (dict(m=65), dict(n=16385), dict(n=1), dict(ldx=2), dict(pre=pre[::-1].copy(), K=2), dict(pre=pre[:1], K=1),
               dict(pens=pens, P=2), dict(G=0)):
        with pytest.raises(ValueError):          # ELFIHIP_ERR_ARG, before any launch
            call(**kw)


# 6 ---------------------------------------------------------------------------------------------------------------
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
    semi = elfi_amd.semiparametric_likelihood()
    # every likelihood the two tools evaluate, against truth
    M, seed = int(gold['sl_M']), int(gold['sl_seed'])
    mats, obs = _ma2_matrices(model, int(gold['sl_n_sim'].max()), M, seed)
    ll = elfi_amd.semi_loglik(mats, obs, prefixes=gold['sl_n_sim'])
    dev = _dev(ll, gold['sl_truth_hi'], gold['sl_truth_lo']).max()
    print('log_SL_stdev likelihoods: max |device-truth| %.2e bound %.2e' % (dev, tol))
    assert dev <= tol
    grid = list(gold['pen_grid'])
    mats, obs = _ma2_matrices(model, int(gold['pen_n_sim'].max()), int(gold['pen_M']), int(gold['pen_seed']))
    ll = elfi_amd.semi_loglik(mats, obs, prefixes=gold['pen_n_sim'], shrinkage='warton', penalties=grid)
    dev = _dev(ll, gold['pen_truth_hi'], gold['pen_truth_lo']).max()
    print('select_penalty likelihoods: max |device-truth| %.2e bound %.2e' % (dev, tol))
    assert dev <= tol
    # the tools themselves: a standard deviation moves by no more than the largest change of a likelihood, which is at
    # most |device - truth| + |reference - truth| <= tol + tol / 16
    std = elfi_amd.log_SL_stdev(model, THETA, list(gold['sl_n_sim']), FEATS, likelihood=semi, M=M, seed=seed)
    assert std.shape == gold['sl_std'].shape and np.abs(std - gold['sl_std']).max() <= tol * 17 / 16
    lm, sd = elfi_amd.select_penalty(model, list(gold['pen_n_sim']), THETA, FEATS, likelihood=semi, lmdas=grid,
                                     M=int(gold['pen_M']), shrinkage='warton', seed=int(gold['pen_seed']))
    assert np.array_equal(lm, gold['pen_lmdas'])
    assert np.abs(sd - gold['pen_stds']).max() <= tol * 17 / 16


@needs_reference
def test_bsl_chain_reproduces_the_reference(hip_ctx, elfi, gold):
    import elfi_amd
    from elfi.examples import ma2
    tol = bound_for(gold, 2)
    n, rnd, seed = int(gold['bsl_n']), int(gold['bsl_round']), int(gold['bsl_seed'])
    hip = elfi_amd.HipBSL(ma2.get_model(seed_obs=4), rnd, feature_names=FEATS,
                          likelihood=elfi_amd.semiparametric_likelihood(), seed=seed)
    assert isinstance(hip, elfi.BSL) and not hip.is_misspec
    res = hip.sample(n, sigma_proposals=0.02 * np.eye(2), params0=THETA, bar=False)
    assert type(res).__name__ == 'BslSample'
    params, logpost = hip.state['params'], hip.state['logposterior']
    moved = np.any(np.diff(params, axis=0) != 0, axis=1)
    ref_moved = np.any(np.diff(gold['bsl_params'], axis=0) != 0, axis=1)
    flips = np.flatnonzero(moved != ref_moved)
    assert flips.size == 0, 'accept/reject differs from the reference first at sample %d (reference logposterior %r, ' \
        'device %r)' % (flips[0] + 1, gold['bsl_logpost'][flips[0] + 1], logpost[flips[0] + 1])
    assert np.abs(params - gold['bsl_params']).max() <= tol * 17 / 16
    assert np.abs(logpost - gold['bsl_logpost']).max() <= tol * 17 / 16
