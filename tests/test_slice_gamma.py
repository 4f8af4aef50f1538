"""CPU: the statement of the gamma slice samplers (tests/slice_gamma_ref.py) against the reference's recorded outputs
(tests/golden/slice_gamma.npz, scripts/make_golden_slice_gamma.py), and the host side of elfi_amd.slice_gamma*: argument
checks, the RandomState bookkeeping of the drop-ins (the device call stubbed by the statement), HipBSL's keyword.

The bound of a log-likelihood with m parameters is 16 x the largest |reference - truth| over the recorded cases with that
m; gamma is a function of w, the draws and the decisions alone, so it must be equal bit for bit."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import slice_gamma_ref as S

ADJ = {S.MEAN: 'mean', S.VARIANCE: 'variance'}
N_CASES = 37


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'slice_gamma.npz'))


def case(gold, k):
    keys = ('y', 'mean', 'cov', 'gamma', 'loglik', 'adj', 'tau', 'w', 'max_iter', 'draws', 'ref_gamma', 'ref_loglik', 'used',
            'evals', 'truth_hi', 'truth_lo', 'margin', 'e_ref')
    c = {key: gold['c%d_%s' % (k, key)] for key in keys}
    for key in ('adj', 'max_iter', 'used', 'evals'):
        c[key] = int(c[key])
    for key in ('loglik', 'tau', 'w', 'ref_loglik', 'truth_hi', 'truth_lo', 'margin', 'e_ref'):
        c[key] = float(c[key])
    c['kind'] = str(gold['kinds'][k])
    return c


def bound_for(gold, m):
    """16 x the largest recorded error of the reference over every case with m adjustment parameters."""
    return float(gold['bound'][list(gold['bound_m']).index(m)])


def error(got, c):
    return abs((got - c['truth_hi']) - c['truth_lo'])


def test_fixture_holds_every_shape_and_case(gold):
    assert int(gold['n_cases']) == N_CASES
    cases = [case(gold, k) for k in range(N_CASES)]
    for m in (1, 2, 15, 16, 17, 33, 64):
        for adj in (S.MEAN, S.VARIANCE):
            assert any(c['gamma'].size == m and c['adj'] == adj and c['kind'] == 'base' for c in cases)
    assert {c['kind'] for c in cases} == {'base', 'corr95', 'far8', 'gamma0'}
    assert {c['max_iter'] for c in cases} == {0, 1, 2, 1000} and {c['w'] for c in cases} == {0.05, 1.0}
    for c in cases:
        assert c['margin'] >= 1e-6 and c['draws'].size >= c['used']
        assert 16.0 * c['e_ref'] <= bound_for(gold, c['gamma'].size)
    for m in gold['bound_m']:
        assert bound_for(gold, m) == 16.0 * max(c['e_ref'] for c in cases if c['gamma'].size == m)


@pytest.mark.parametrize('k', range(N_CASES))
def test_statement_against_the_reference(gold, k):
    c = case(gold, k)
    g, ll, used, evals, margin = S.slice_gamma(c['adj'], c['y'], c['mean'], c['cov'], c['gamma'], c['loglik'], c['tau'], c['w'],
                                               c['max_iter'], c['draws'])
    assert np.array_equal(np.array(g), c['ref_gamma'])
    assert (used, evals) == (c['used'], c['evals'])
    assert margin >= 1e-6 / 2
    assert error(float(ll), c) <= bound_for(gold, c['gamma'].size)
    if c['max_iter'] == 0:      # nothing can be accepted: the input comes back
        assert np.array_equal(c['ref_gamma'], c['gamma']) and c['ref_loglik'] == c['loglik']


def test_the_draws_are_the_legacy_generators():
    """exponential(1) = -log(1 - d) and uniform(a, b) = a + (b - a) d of the double random_sample() returns."""
    a, b = np.random.RandomState(11), np.random.RandomState(11)
    for i in range(200):
        lo, hi = -1.5 + 0.01 * i, 0.3 + 0.07 * i
        d = b.random_sample()
        if i % 2:
            assert a.exponential(1) == -math.log(1.0 - d)
        else:
            assert a.uniform(lo, hi) == lo + (hi - lo) * d
    buffered = S.BufferedRandomState(np.random.RandomState(11).random_sample(4))
    c = np.random.RandomState(11)
    assert buffered.exponential(1) == c.exponential(1) and buffered.uniform(-2.0, 3.0) == c.uniform(-2.0, 3.0)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    rs = np.random.RandomState(0)
    m = 3
    y, mean, cov, gamma, u = rs.randn(m), rs.randn(m), np.eye(m), np.zeros(m), rs.rand(50)
    ok = dict(adjustment='mean', draws=u)
    bad = [dict(ok, adjustment='median'), dict(ok, tau=0.0), dict(ok, tau=-1.0), dict(ok, w=0.0), dict(ok, w=float('nan')),
           dict(ok, max_iter=-1), dict(ok, max_iter=(1 << 20) + 1), dict(ok, draws=None), dict(ok, seed=3),
           dict(ok, draws=rs.rand(2, 50)), dict(ok, n_groups=2)]
    for kw in bad:
        with pytest.raises(ValueError):
            elfi_amd.slice_gamma(y, -3.0, gamma, mean, cov, **kw)
    with pytest.raises(ValueError):
        elfi_amd.slice_gamma(y, -3.0, np.zeros(65), np.zeros(65), np.eye(65), **ok)
    with pytest.raises(ValueError):
        elfi_amd.slice_gamma(y, -3.0, gamma, mean, np.eye(4), **ok)
    with pytest.raises(ValueError):
        elfi_amd.slice_gamma(y, [-3.0, -2.0], gamma, mean, cov, **ok)
    with pytest.raises(ValueError):
        elfi_amd.slice_gamma_mean(y, [-3.0, -2.0], gamma, mean, cov)
    with pytest.raises(AssertionError, match='device context'):      # ... and a good call does get that far
        elfi_amd.slice_gamma(y, -3.0, gamma, mean, cov, **ok)


class StatementContext:
    """Stands in for the device context: `call('elfihip_slice_gamma', ...)` runs the statement on the arguments."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def _array(addr, count, ctype=C.c_double):
        return np.ctypeslib.as_array((ctype * count).from_address(addr))

    def call(self, name, adjustment, G, m, y, mean, cov, ldc, gamma_in, loglik_in, tau, w, max_iter, U, n_u, seed, stream,
             gamma_out, loglik_out, used, evals, status):
        assert name == 'elfihip_slice_gamma' and ldc == m and U
        self.calls.append(n_u)
        for g in range(G):
            row = lambda p, n=m: self._array(p + 8 * g * n, n)
            out = S.slice_gamma_status(adjustment, row(y), row(mean), row(cov, m * m).reshape(m, m), row(gamma_in),
                                       row(loglik_in, 1)[0], tau, w, max_iter, row(U, n_u))
            row(gamma_out)[:] = out[0]
            row(loglik_out, 1)[0] = out[1]
            self._array(used + 8 * g, 1, C.c_int64)[0] = out[2]
            self._array(evals + 8 * g, 1, C.c_int64)[0] = out[3]
            self._array(status + 4 * g, 1, C.c_int32)[0] = out[4]


@pytest.fixture
def statement_ctx(monkeypatch):
    from elfi_amd import _lib
    ctx = StatementContext()
    monkeypatch.setattr(_lib, 'default_context', lambda *a, **k: ctx)
    return ctx


@pytest.mark.parametrize('k', [4, 10, 12, 24])      # m = 2 mean, m = 15 variance, m = 16 mean, corr95 mean
@pytest.mark.parametrize('first', [None, 2])
def test_drop_ins_leave_the_generator_where_the_reference_would(gold, statement_ctx, monkeypatch, k, first):
    import elfi_amd
    from elfi_amd import synlik
    c = case(gold, k)
    if first is not None:
        monkeypatch.setattr(synlik, '_first_draws', lambda m: first)
    fn = {S.MEAN: elfi_amd.slice_gamma_mean, S.VARIANCE: elfi_amd.slice_gamma_variance}[c['adj']]
    args = (c['y'], c['loglik'], c['gamma'], c['mean'], c['cov'])
    kw = dict(tau=c['tau'], w=c['w'], max_iter=c['max_iter'])
    seed = 77
    draws = np.random.RandomState(seed).random_sample(4096)
    want = S.slice_gamma(c['adj'], c['y'], c['mean'], c['cov'], c['gamma'], c['loglik'], c['tau'], c['w'], c['max_iter'], draws)

    rs = np.random.RandomState(seed)
    rs.standard_normal()                  # (leaves a cached normal in the state: it must survive)
    cached = rs.get_state()[3:]
    rs.set_state(np.random.RandomState(seed).get_state()[:3] + cached)
    g, ll = fn(*args, random_state=rs, **kw)
    assert np.array_equal(g, np.array(want[0])) and ll == want[1] and isinstance(ll, np.float64)
    assert rs.get_state()[3:] == cached
    assert rs.random_sample() == draws[want[2]]          # the next double is the one after the sweep's last
    if first is not None:
        assert len(statement_ctx.calls) > 1 and statement_ctx.calls[0] == 2 and want[2] > 2
        assert all(b == 4 * a for a, b in zip(statement_ctx.calls, statement_ctx.calls[1:]))
    else:
        assert statement_ctx.calls == [8 * c['gamma'].size + 16]

    np.random.seed(seed)                  # random_state=None: NumPy's global generator, as in the reference
    g2, ll2 = fn(*args, **kw)
    assert np.array_equal(g2, g) and ll2 == ll and np.random.random_sample() == draws[want[2]]


SINGULAR = np.array([[4.0, 4.0, 0.0], [4.0, 4.0, 0.0], [0.0, 0.0, 1.0]])      # a repeated column: the second pivot is 4 - 2 2


def test_drop_in_raises_where_the_covariance_has_no_factor(statement_ctx):
    import elfi_amd
    rs = np.random.RandomState(9)
    before = rs.get_state()[1].copy()
    with pytest.raises(FloatingPointError):
        elfi_amd.slice_gamma_mean(np.ones(3), -5.0, np.zeros(3), np.zeros(3), SINGULAR, random_state=rs)
    assert np.array_equal(rs.get_state()[1], before)         # no draw was taken before the factorisation failed


def test_batched_call_shapes(statement_ctx, gold):
    import elfi_amd
    c = case(gold, 4)
    m = c['gamma'].size
    G = 3
    tile = lambda a: np.broadcast_to(a, (G,) + np.shape(a)).copy()
    g, ll, used, evals, status = elfi_amd.slice_gamma(c['y'], tile(c['loglik']), tile(c['gamma']), tile(c['mean']), tile(c['cov']),
                                                      ADJ[c['adj']], tau=c['tau'], w=c['w'], max_iter=c['max_iter'],
                                                      draws=tile(c['draws']), return_info=True)
    assert g.shape == (G, m) and ll.shape == (G,) and used.dtype == np.int64 and status.dtype == np.int32
    assert np.array_equal(g, tile(c['ref_gamma'])) and list(used) == [c['used']] * G and list(evals) == [c['evals']] * G
    one = elfi_amd.slice_gamma(c['y'], c['loglik'], c['gamma'], c['mean'], c['cov'], ADJ[c['adj']], tau=c['tau'], w=c['w'],
                               max_iter=c['max_iter'], draws=c['draws'][:2], return_info=True)
    assert one[0].shape == (m,) and np.all(np.isnan(one[0])) and np.isnan(one[1]) and one[2] == 2 and one[4] == S.OUT_OF_DRAWS


@pytest.fixture(scope='module')
def elfi():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'oracle'))
    import ref_shim
    if not ref_shim.available():
        pytest.skip('no reference package (run oracle/make_ref.sh)')
    e = ref_shim.install()
    import elfi.clients.native as native
    native.set_as_default()
    return e


def test_hip_bsl_keyword(elfi):
    import elfi_amd
    from functools import partial
    from elfi.examples import ma2
    from elfi.methods.bsl.slice_gamma_variance import slice_gamma_variance as reference_sampler
    model = ma2.get_model(seed_obs=4)
    feats = ['S1', 'S2']
    with pytest.raises(ValueError, match='gamma_sampler'):
        elfi_amd.HipBSL(model, 50, feature_names=feats, likelihood=elfi_amd.robust_likelihood('mean'), gamma_sampler='host')
    with pytest.raises(ValueError, match='robust'):
        elfi_amd.HipBSL(model, 50, feature_names=feats, gamma_sampler='device')
    with pytest.raises(ValueError, match='robust'):
        elfi_amd.HipBSL(model, 50, feature_names=feats, likelihood=elfi_amd.standard_likelihood(), gamma_sampler='device')
    for adjustment, fn in (('mean', elfi_amd.slice_gamma_mean), ('variance', elfi_amd.slice_gamma_variance)):
        bsl = elfi_amd.HipBSL(model, 50, feature_names=feats, likelihood=elfi_amd.robust_likelihood(adjustment),
                              gamma_sampler='device', seed=1)
        sampler, gamma0 = bsl._resolve_gamma_sampler(0.25, 2.0, 7)
        assert isinstance(sampler, partial) and sampler.func is fn
        assert sampler.keywords == dict(tau=0.25, w=2.0, max_iter=7, random_state=bsl.random_state)
        assert np.array_equal(gamma0, np.repeat(0.0 if adjustment == 'mean' else 0.25, 2))
    default = elfi_amd.HipBSL(model, 50, feature_names=feats, likelihood=elfi_amd.robust_likelihood('variance'), seed=1)
    assert default._resolve_gamma_sampler(0.5, 1.0, 1000)[0].func is reference_sampler
