"""GPU: graphical-lasso shrinkage (csrc/glasso.hip through elfi_amd/synlik.py).

The yardstick is the converged NumPy statement (tests/glasso_ref.py) recorded in tests/golden/glasso.npz; the bound per
case is 16 x the disagreement of that statement with scikit-learn's solver at its tightest converging tolerance, floored
at the standard likelihood's bound for the nearest m (scripts/make_golden_glasso.py).  What is the same arithmetic (groups
and penalties in one call against single calls, the device-pointer form) must be equal bit for bit.
Measured on an MI355X: DESIGN.md, "Graphical-lasso shrinkage".
"""
import os
import sys
import warnings

import numpy as np
import pytest

import glasso_ref as R

ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle')
sys.path.insert(0, ORACLE)
import ref_shim  # noqa: E402

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')
THETA, FEATS = [0.6, 0.2], ['S1', 'S2']


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'glasso.npz'))


@pytest.fixture(scope='module')
def elfi():
    e = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    return e


# 1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci', range(5))
def test_solver_against_the_converged_statement(hip_ctx, gold, ci):
    import elfi_amd
    S, alphas, m = gold['S_%d' % ci], gold['alphas'][ci], R.CASES[ci][2]
    W, Theta, n_iter, status = elfi_amd.graphical_lasso(S, list(alphas), return_n_iter=True, return_status=True)
    err = np.abs(W - gold['W_%d' % ci]).max(axis=(1, 2)) / np.diag(S).max()
    print('m=%d sweeps %s |device-ref| / max diag %s bound %s' % (m, n_iter, err, gold['bound_W'][ci]))
    assert np.all(status == 1)
    assert np.all(err <= gold['bound_W'][ci])
    assert np.array_equal(W[0], S)
    off = ~np.eye(m, dtype=bool)
    for p in range(len(alphas)):
        assert np.array_equal(np.diag(W[p]), np.diag(S))
    assert np.all(W[-1][off] == 0) and np.all(Theta[-1][off] == 0)


# 2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ci,form', [(ci, f) for ci in range(5) for f in ('plain', 'standardise')] + [(2, 'whitening')])
def test_loglik_against_the_statement(hip_ctx, gold, ci, form):
    import elfi_amd
    X, y, Wh = R.make_case(*R.CASES[ci])
    kw = dict(standardise=True) if form == 'standardise' else dict(whitening=Wh) if form == 'whitening' else {}
    ll, status = elfi_amd.glasso_loglik(X, y, penalties=R.LOGLIK_ALPHAS, return_status=True, **kw)
    want, bound = gold['ll_' + form][ci], gold['bound_ll_' + form][ci]
    print('m=%d %s device %s |device-ref| %s bound %s' % (R.CASES[ci][2], form, ll, np.abs(ll - want), bound))
    assert np.all(status == 1) and np.all(np.abs(ll - want) <= bound)


# 3 ---------------------------------------------------------------------------------------------------------------
def test_groups_penalties_and_the_device_form_equal_single_calls(hip_ctx):
    import torch
    import elfi_amd
    from elfi_amd import _lib
    G, n, m = 3, 40, 17
    X, y, Wh = R.make_case(33, G * n, m)
    pens = np.array(R.LOGLIK_ALPHAS)
    ll, mean, cov, status = elfi_amd.glasso_loglik(X, y, penalties=pens, n_groups=G, whitening=Wh, return_moments=True,
                                                   return_status=True)
    assert ll.shape == (G, 3) and cov.shape == (G, 3, m, m) and np.all(status == 1)
    for g in range(G):
        for p in range(3):
            one, m1, c1 = elfi_amd.glasso_loglik(X[g * n:(g + 1) * n], y, penalty=pens[p], whitening=Wh, return_moments=True)
            assert one == ll[g, p] and np.array_equal(m1[0], mean[g]) and np.array_equal(c1[0], cov[g, p])
    ldx, dev = m + 5, torch.device('cuda')
    wide = np.full((G * n, ldx), np.nan)
    wide[:, :m] = X
    dX, dy, dWh = (torch.from_numpy(a).to(dev) for a in (wide, y, Wh))
    dll = torch.zeros((G, 3), dtype=torch.float64, device=dev)
    dst = torch.zeros((G, 3), dtype=torch.int32, device=dev)
    dmean = torch.zeros((G, m), dtype=torch.float64, device=dev)
    dcov = torch.zeros((G, 3, m, m), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    hip_ctx.call("elfihip_syn_loglik_glasso_dev", dX.data_ptr(), G, n, m, ldx, dy.data_ptr(), dWh.data_ptr(), _lib.ptr(pens),
                 3, 0, 1e-12, 10000, dll.data_ptr(), dst.data_ptr(), dmean.data_ptr(), dcov.data_ptr())
    hip_ctx.synchronize()
    assert np.array_equal(dll.cpu().numpy(), ll) and np.array_equal(dst.cpu().numpy(), status)
    assert np.array_equal(dmean.cpu().numpy(), mean) and np.array_equal(dcov.cpu().numpy(), cov)


# 4 ---------------------------------------------------------------------------------------------------------------
def test_the_iteration_cap_is_reported_once(hip_ctx, gold):
    import elfi_amd
    S = gold['S_2']
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        W, Theta, n_iter, status = elfi_amd.graphical_lasso(np.stack([S, S]), R.FIXED_ALPHAS[1], max_iter=1,
                                                            return_n_iter=True, return_status=True)
    assert len(caught) == 1 and '2 of 2' in str(caught[0].message)
    assert np.all(status == 2) and np.all(n_iter == 1) and np.all(np.isfinite(W)) and np.all(np.isfinite(Theta))


# 5, 6 ------------------------------------------------------------------------------------------------------------
@needs_reference
def test_select_glasso_penalty_is_the_rule_on_the_batched_likelihoods(hip_ctx, elfi):
    import elfi_amd
    from elfi_amd.synlik import _generate_groups
    model = elfi_amd.ma2_model(seed_obs=4)
    lmdas, M, n_sim, seed = [0.005, 0.02, 0.08, 0.3], 5, 100, 7
    theta = {'t1': np.full(n_sim, THETA[0]), 't2': np.full(n_sim, THETA[1])}     # the device simulator takes its batch from these
    groups, obs = _generate_groups(model, theta, n_sim, FEATS, M, seed)
    ll = elfi_amd.glasso_loglik(groups, obs, penalties=lmdas)
    assert ll.shape == (M, 4) and np.all(np.isfinite(ll))
    for i in range(M):
        assert np.array_equal(elfi_amd.glasso_loglik(groups[i], obs, penalties=lmdas), ll[i])
    std = np.array([np.std(ll[:, j]) for j in range(4)])
    pick = np.argmin(np.abs(std - 1.5))
    got = elfi_amd.select_glasso_penalty(model, n_sim, theta, FEATS, lmdas=lmdas, M=M, seed=seed)
    assert np.array_equal(got[0], [lmdas[pick]]) and np.array_equal(got[1], [std[pick]])


@needs_reference
def test_bsl_chain_with_the_glasso_likelihood(hip_ctx, elfi):
    import elfi_amd
    from elfi.examples import ma2
    bsl = elfi.BSL(ma2.get_model(seed_obs=4), 100, feature_names=FEATS, likelihood=elfi_amd.glasso_likelihood(0.05), seed=3)
    bsl.sample(20, sigma_proposals=0.02 * np.eye(2), params0=THETA, bar=False)
    assert len(bsl.state['logposterior']) >= 20 and np.all(np.isfinite(bsl.state['logposterior']))
