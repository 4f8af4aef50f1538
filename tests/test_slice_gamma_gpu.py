"""GPU: the gamma slice samplers (csrc/slice_gamma.hip through elfi_amd.slice_gamma*).

The yardstick is tests/golden/slice_gamma.npz (scripts/make_golden_slice_gamma.py): the reference's own functions fed with
a recorded buffer of draws, and the statement in 50-digit arithmetic (`truth`).  gamma is a function of w, the draws and
the decisions alone and every recorded case has settled decisions (margin >= 1e-6), so gamma, the draws consumed and the
evaluations made must EQUAL the reference's; the returned log-likelihood must lie within 16 x max |reference - truth| over
the recorded cases with the same m.  What is the same arithmetic (a problem alone against the same problem among others,
the generator in the kernel against the same uniforms from a buffer, the _dev form against the host form) must be equal
bit for bit.

Measured on an MI355X (|device - truth| per case against |reference - truth|): see DESIGN.md, "The slice samplers for
gamma".
"""
import ctypes as C
import os

import numpy as np
import pytest

import philox_ref as PH
import slice_gamma_ref as S
import stream_order as SO
from test_slice_gamma import ADJ, N_CASES, SINGULAR, bound_for, case, error
from test_synlik_gpu import FEATS, THETA, elfi, needs_reference  # noqa: F401  (elfi is a fixture)

pytestmark = pytest.mark.gpu

I64, U64, DBL = C.c_int64, C.c_uint64, C.c_double


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'slice_gamma.npz'))


def run(c, **kw):
    import elfi_amd
    args = dict(tau=c['tau'], w=c['w'], max_iter=c['max_iter'], draws=c['draws'], return_info=True)
    args.update(kw)
    return elfi_amd.slice_gamma(c['y'], c['loglik'], c['gamma'], c['mean'], c['cov'], ADJ[c['adj']], **args)


@pytest.mark.parametrize('k', range(N_CASES))
def test_recorded_case(hip_ctx, gold, k):
    c = case(gold, k)
    m = c['gamma'].size
    g, ll, used, evals, status = run(c)
    tol = bound_for(gold, m)
    print('%-7s %-8s m %2d w %.2f max_iter %4d: used %d (%d) evals %d (%d) |reference-truth| %.2e |device-truth| %.2e bound %.2e'
          % (c['kind'], ADJ[c['adj']], m, c['w'], c['max_iter'], used, c['used'], evals, c['evals'], c['e_ref'], error(ll, c), tol))
    assert status == S.OK
    assert (used, evals) == (c['used'], c['evals'])
    assert np.array_equal(g, c['ref_gamma'])
    assert error(ll, c) <= tol
    if c['max_iter'] == 0:
        assert ll == c['loglik']


def _mixed(gold, k, G=8):
    """G problems with the settings of recorded case k: its own and perturbed copies, each with draws of its own."""
    c = case(gold, k)
    m = c['gamma'].size
    rs = np.random.RandomState(900 + k)
    std = np.sqrt(np.diag(c['cov']))
    probs = dict(y=np.empty((G, m)), mean=np.empty((G, m)), cov=np.empty((G, m, m)), gamma=np.empty((G, m)), loglik=np.empty(G),
                 draws=rs.random_sample((G, 64 * m + 512)))
    for g in range(G):
        scale = 1.0 if g == 0 else rs.uniform(0.5, 2.0, m)
        probs['cov'][g] = c['cov'] * np.outer(scale, scale)
        probs['mean'][g] = c['mean'] + (g > 0) * rs.randn(m)
        probs['y'][g] = probs['mean'][g] + (c['y'] - c['mean']) * scale + (g > 0) * 0.5 * std * scale * rs.randn(m)
        probs['gamma'][g] = c['gamma'] if g == 0 else (rs.laplace(0, 0.3, m) if c['adj'] == S.MEAN else rs.exponential(0.5, m))
        sd = np.sqrt(np.diag(probs['cov'][g]))
        if g == 0:
            probs['loglik'][g] = c['loglik']
        elif c['adj'] == S.MEAN:        # the log-likelihood of the state, as a chain would hold it
            probs['loglik'][g] = S.F64.logpdf(list(probs['y'][g] - (probs['mean'][g] + sd * probs['gamma'][g])), probs['cov'][g].tolist())
        else:
            probs['loglik'][g] = S.F64.logpdf(list(probs['y'][g] - probs['mean'][g]),
                                              (probs['cov'][g] + np.diag((sd * probs['gamma'][g]) ** 2)).tolist())
    probs['draws'][0, :c['draws'].size] = c['draws']
    return c, probs


def _call(c, p, rows=None, **kw):
    import elfi_amd
    sl = slice(None) if rows is None else rows
    args = dict(tau=c['tau'], w=c['w'], max_iter=c['max_iter'], draws=p['draws'][sl], return_info=True)
    args.update(kw)
    return elfi_amd.slice_gamma(p['y'][sl], p['loglik'][sl], p['gamma'][sl], p['mean'][sl], p['cov'][sl], ADJ[c['adj']], **args)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize('k', [8, 10, 20, 21])      # m = 15 and m = 33, both adjustments
def test_a_problem_does_not_depend_on_the_others(hip_ctx, gold, k):
    c, p = _mixed(gold, k)
    G = p['loglik'].size
    g, ll, used, evals, status = _call(c, p)
    assert np.all(status == S.OK)
    assert np.array_equal(g[0], c['ref_gamma']) and used[0] == c['used'] and evals[0] == c['evals']
    assert len({tuple(row) for row in g}) == G
    for i in range(G):
        one = _call(c, p, rows=slice(i, i + 1))
        for a, b in zip(one, (g[i:i + 1], ll[i:i + 1], used[i:i + 1], evals[i:i + 1], status[i:i + 1])):
            assert np.array_equal(_bits(a), _bits(b)), 'problem %d differs between a call of its own and the call of %d' % (i, G)


@pytest.mark.parametrize('k', [9, 11])      # m = 15, both adjustments
def test_out_of_draws_and_nonfinite_leave_the_other_problems_alone(hip_ctx, gold, k):
    c, p = _mixed(gold, k)
    G, m = p['gamma'].shape
    full = _call(c, p)
    assert np.all(full[4] == S.OK)
    n_u = int(np.sort(full[2])[G // 2 - 1])            # the buffer ends for the problems that need more than that
    assert full[2].min() <= n_u < full[2].max()
    short = dict(p, draws=p['draws'][:, :n_u].copy())
    bad = 1 if full[2][1] <= n_u else int(np.flatnonzero(full[2] <= n_u)[0])
    short['cov'] = p['cov'].copy()
    short['cov'][bad] = np.eye(m)
    short['cov'][bad][:3, :3] = SINGULAR              # a repeated column: the second pivot is exactly zero
    short['gamma'] = p['gamma'].copy()
    short['gamma'][bad] = 0.0                         # (the variance form adds nothing to the diagonal)
    g, ll, used, evals, status = _call(c, short)
    for i in range(G):
        if i == bad:
            assert status[i] == S.NONFINITE and np.all(np.isnan(g[i])) and np.isnan(ll[i])
        elif full[2][i] > n_u:
            assert status[i] == S.OUT_OF_DRAWS and np.all(np.isnan(g[i])) and np.isnan(ll[i]) and used[i] == n_u
        else:
            assert status[i] == S.OK and used[i] == full[2][i] and evals[i] == full[3][i]
            assert np.array_equal(_bits(g[i]), _bits(full[0][i])) and ll[i] == full[1][i]
    assert (status == S.OUT_OF_DRAWS).sum() >= 1 and (status == S.OK).sum() >= 1


@pytest.mark.parametrize('k', [5, 19])      # m = 2 mean, m = 17 variance
def test_the_generator_in_the_kernel_is_the_buffer_of_its_uniforms(hip_ctx, gold, k):
    import elfi_amd
    from elfi_amd.priors import SLICE_GAMMA_STREAM_BASE
    c, p = _mixed(gold, k, G=3)
    seed = 20250 + k
    n_u = p['draws'].shape[1]
    U = np.stack([PH.uniform53_first(seed, SLICE_GAMMA_STREAM_BASE + g, np.arange(n_u, dtype=np.uint64)) for g in range(3)])
    assert U.min() >= 0.0 and U.max() < 1.0
    buffered = _call(c, dict(p, draws=U))
    drawn = _call(c, p, draws=None, seed=seed)
    assert np.all(buffered[4] == S.OK) and buffered[2].max() < n_u
    for a, b in zip(buffered, drawn):
        assert np.array_equal(_bits(a), _bits(b))


def test_argument_errors_of_the_library(hip_ctx):
    m = 3
    z = np.zeros(m * m + 8)
    out = np.zeros(16)
    cnt = np.zeros(4, dtype=np.int64)
    st = np.zeros(4, dtype=np.int32)

    def rc(adjustment=0, G=1, m=m, ldc=m, tau=0.5, w=1.0, max_iter=10):
        return hip_ctx.lib.elfihip_slice_gamma(hip_ctx.handle, adjustment, G, m, z.ctypes.data, z.ctypes.data, z.ctypes.data, ldc,
                                               z.ctypes.data, z.ctypes.data, tau, w, max_iter, z.ctypes.data, 8, 0, 0,
                                               out.ctypes.data, out.ctypes.data, cnt.ctypes.data, cnt.ctypes.data, st.ctypes.data)
    for kw in (dict(adjustment=2), dict(adjustment=-1), dict(m=0), dict(m=65, ldc=65), dict(ldc=m - 1), dict(tau=0.0), dict(w=0.0),
               dict(tau=float('nan')), dict(max_iter=-1), dict(max_iter=(1 << 20) + 1), dict(G=-1)):
        assert rc(**kw) == 1, kw
    assert not out.any() and not cnt.any() and not st.any()
    assert rc(G=0) == 0


def _dev_case(c, p):
    """The _dev form with the covariances at pitch m + 3, every input from a base that is only 8-byte aligned, the results
    between guard words."""
    G, m = p['gamma'].shape
    ldc = m + 3
    n_u = p['draws'].shape[1]

    def odd(a):
        return np.concatenate([[np.nan], np.ascontiguousarray(a, dtype=np.float64).reshape(-1)])

    def case_fn(d):
        cov = np.full((G * m, ldc), np.nan)
        cov[:, :m] = p['cov'].reshape(G * m, m)
        ins = [d.input(odd(a), first=1) for a in (p['y'], p['mean'], cov, p['gamma'], p['loglik'], p['draws'])]
        g_out, ll_out = d.out(G, m), d.out(G)
        import torch
        used, evals, status = d.out_raw(G, torch.int64), d.out_raw(G, torch.int64), d.out_raw(G, torch.int32)
        d.go()
        d.call('elfihip_slice_gamma_dev', d.cx, c['adj'], I64(G), m, ins[0].ptr, ins[1].ptr, ins[2].ptr, I64(ldc), ins[3].ptr,
               ins[4].ptr, DBL(c['tau']), DBL(c['w']), I64(c['max_iter']), ins[5].ptr, I64(n_u), U64(0), U64(0), g_out.ptr,
               ll_out.ptr, used.ptr, evals.ptr, status.ptr)
        d.done()
    return case_fn


@pytest.mark.parametrize('k', [12, 15])      # m = 16 mean and variance: pitch 19, odd base
def test_dev_form_at_the_callers_pitch_on_a_busy_stream(hip_ctx, gold, k):
    c, p = _mixed(gold, k, G=4)
    G, m = p['gamma'].shape
    name = 'slice_gamma %s' % ADJ[c['adj']]
    ref, got, d = SO.run_both(hip_ctx, _dev_case(c, p), name)
    SO.guards_intact(ref, d.guarded)
    SO.guards_intact(got, d.guarded)
    SO.assert_same(ref, got, name)
    assert d.still_busy, '%s: the stream was idle when the call had returned: it waited for the stream on the host' % name
    host = _call(c, p)
    lead = SO._LEAD
    assert np.array_equal(got['out0'].view(np.float64)[lead:lead + G * m], host[0].reshape(-1))
    assert np.array_equal(got['out1'].view(np.float64)[lead:lead + G], host[1])
    assert np.array_equal(got['out2'][:8 * G].view(np.int64), host[2]) and np.all(got['out2'][8 * G:] == 0xA5)
    assert np.array_equal(got['out3'][:8 * G].view(np.int64), host[3]) and np.all(got['out3'][8 * G:] == 0xA5)
    assert np.array_equal(got['out4'][:4 * G].view(np.int32), host[4]) and np.all(got['out4'][4 * G:] == 0xA5)
    assert np.array_equal(host[0][0], c['ref_gamma'])


def test_drop_ins_follow_the_reference_and_its_generator(hip_ctx, gold):
    import elfi_amd
    for k in (6, 16):      # m = 2 variance, m = 17 mean
        c = case(gold, k)
        fn = {S.MEAN: elfi_amd.slice_gamma_mean, S.VARIANCE: elfi_amd.slice_gamma_variance}[c['adj']]
        seed = 31 + k
        draws = np.random.RandomState(seed).random_sample(4096)
        want = S.slice_gamma(c['adj'], c['y'], c['mean'], c['cov'], c['gamma'], c['loglik'], c['tau'], c['w'], c['max_iter'], draws)
        assert want[4] >= 1e-6           # (settled with this generator's draws: 5.0e-2 and 2.6e-4)
        rs = np.random.RandomState(seed)
        g, ll = fn(c['y'], c['loglik'], c['gamma'], c['mean'], c['cov'], tau=c['tau'], w=c['w'], max_iter=c['max_iter'],
                   random_state=rs)
        assert np.array_equal(g, np.array(want[0])) and abs(ll - want[1]) <= 2 * bound_for(gold, c['gamma'].size)   # both within the bound of the truth
        assert rs.random_sample() == draws[want[2]]
    with pytest.raises(FloatingPointError):
        elfi_amd.slice_gamma_mean(np.ones(3), -5.0, np.zeros(3), np.zeros(3), SINGULAR, random_state=np.random.RandomState(1))


@needs_reference
@pytest.mark.parametrize('adjustment', ['variance', 'mean'])
def test_rbsl_chain_reproduces_the_reference(hip_ctx, elfi, gold, adjustment):
    """The device likelihood and the device gamma sampler in the reference's chain: the same accept/reject decisions, and
    gamma and the logposterior within the bound of m = 2."""
    import elfi_amd
    from elfi.examples import ma2
    n, rnd, seed = int(gold['chain_n']), int(gold['chain_round']), int(gold['chain_seed'])
    tol_gamma = tol_ll = bound_for(gold, 2)
    bsl = elfi_amd.HipBSL(ma2.get_model(seed_obs=4), rnd, feature_names=FEATS, likelihood=elfi_amd.robust_likelihood(adjustment),
                          gamma_sampler='device', seed=seed)
    bsl.sample(n, sigma_proposals=0.02 * np.eye(2), params0=THETA, bar=False)
    ref_params, ref_logpost, ref_gamma = (gold['chain_%s_%s' % (adjustment, key)] for key in ('params', 'logpost', 'gamma'))
    moved = np.any(np.diff(bsl.state['params'], axis=0) != 0, axis=1)
    ref_moved = np.any(np.diff(ref_params, axis=0) != 0, axis=1)
    print('R-BSL chain (%s): max |gamma - reference| %.2e (bound %.2e), max |logposterior - reference| %.2e (bound %.2e)'
          % (adjustment, np.abs(bsl.state['gamma'] - ref_gamma).max(), tol_gamma,
             np.abs(bsl.state['logposterior'] - ref_logpost).max(), tol_ll))
    assert np.array_equal(moved, ref_moved)
    assert np.abs(bsl.state['params'] - ref_params).max() <= tol_gamma
    assert np.abs(bsl.state['gamma'] - ref_gamma).max() <= tol_gamma
    assert np.abs(bsl.state['logposterior'] - ref_logpost).max() <= tol_ll
