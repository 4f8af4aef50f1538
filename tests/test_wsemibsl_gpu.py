"""GPU: the batched whitened semiparametric synthetic likelihood (csrc/wsemibsl.hip through elfi_amd/synlik.py).

The yardstick of every log-likelihood is `truth` of tests/golden/wsemibsl.npz, the bound that of tests/test_wsemibsl.py
(bound_for); quantities that are the same sums (one call against single calls, the device-pointer form against the host
form) must be equal bit for bit.  Measured figures: DESIGN.md, "Whitened semiparametric likelihood"."""
import os

import numpy as np
import pytest

import device_layout as DL
import wsemibsl_ref as R
from test_wsemibsl import bound_for

pytestmark = pytest.mark.gpu
WARTON = dict(shrinkage='warton', penalty=0.4)


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'wsemibsl.npz'))


@pytest.mark.parametrize('vi', range(len(R.variants())))
def test_parity_with_truth(hip_ctx, gold, vi):
    import elfi_amd
    ci, tied = R.variants()[vi]
    X, y, W = R.make_case(ci, tied)
    tol = bound_for(gold, X.shape[1])
    devs = []
    for ki, kw in enumerate(({}, WARTON)):
        got = elfi_amd.wsemi_loglik(X, y, W, **kw)
        dev = abs((got - gold['truth_hi'][vi, ki]) - gold['truth_lo'][vi, ki])
        devs.append(float(dev))
    assert max(devs) <= tol, (devs, tol)


@pytest.mark.parametrize('ci,tied', [(2, True), (4, True), (7, False)])
def test_stages(hip_ctx, gold, golden_dir, ci, tied):
    import elfi_amd
    X, y, W = R.make_case(ci, tied)
    n, m = X.shape
    vi = R.variants().index((ci, tied))
    ll, u, rho, scale, scores = elfi_amd.wsemi_loglik(X, y, W, return_parts=True)
    assert u.shape == (1, m) and rho.shape == (1, m, m) and scale.shape == (1, m) and scores.shape == (1, n, m)
    _, u_np, rho_np, d_np, Q2, T = R.wparts(X, y, W)
    assert np.abs(u[0] - u_np).max() <= 1e-15                       # the bound of tests/test_semibsl_gpu.py
    # equal wherever the statement's ranks are; the score bound of tests/test_semibsl_gpu.py (16 x ndtri's recorded error)
    semi = np.load(os.path.join(golden_dir, 'semibsl.npz'))
    yard = 16.0 * max(semi['ppf_%d_ndtri_rel' % k].max() for k in R.S.SCORE_TABLES)
    for j in range(m):
        assert np.array_equal(np.argsort(scores[0][:, j], kind='stable'), np.argsort(T[:, j], kind='stable')), j
    nz = Q2 != 0.0
    assert np.all(scores[0][~nz] == 0.0) and np.abs(scores[0][nz] / Q2[nz] - 1.0).max() <= yard
    assert np.array_equal(rho[0], rho[0].T) and np.all(np.diag(rho[0]) == 1.0)
    e_rho, e_d = np.abs(rho[0] - gold['rho'][vi, :m, :m]).max(), np.abs(scale[0] - gold['scale'][vi, :m]).max()
    print('n=%d m=%d |device-truth| rho %.2e scale %.2e' % (n, m, e_rho, e_d))
    assert e_rho <= bound_for(gold, m, 'e_rho') and e_d <= bound_for(gold, m, 'e_scale')


@pytest.mark.parametrize('ci,tied', [(4, True), (6, False)])
def test_prefixes_penalties_and_groups_in_one_call_equal_single_calls(hip_ctx, ci, tied):
    import elfi_amd
    X, y, W = R.make_case(ci, tied)
    n = len(X)
    pre = [31, 33, n] if n == 257 else [40, 65, n]
    pens = [0.0, 0.4, 1.0]
    rs = np.random.RandomState(7)
    groups = np.stack([X, X[rs.permutation(n)], X[::-1] + 0.25])
    both = elfi_amd.wsemi_loglik(groups, y, W, prefixes=pre, shrinkage='warton', penalties=pens)
    assert both.shape == (3, 3, 3) and np.all(np.isfinite(both))
    for (g, k, j), got in np.ndenumerate(both):
        assert got == elfi_amd.wsemi_loglik(groups[g, :pre[k]], y, W, shrinkage='warton', penalty=pens[j]), (g, k, j)


def test_minus_infinity_cases_leave_the_status_and_the_other_groups_alone(hip_ctx):
    import elfi_amd
    from elfi_amd import _lib
    X, y, W = R.make_case(4)
    far = y.copy()
    far[0] += 60 * X[:, 0].std()
    ll, u, rho, scale, scores = elfi_amd.wsemi_loglik(X, far, W, return_parts=True)
    assert ll == -np.inf and u[0, 0] == 1.0 and np.all(np.isfinite(scale))
    const = X[:100].copy()
    const[:, 2] = 1.0
    assert elfi_amd.wsemi_loglik(X[:2], y, W) == -np.inf
    assert elfi_amd.wsemi_loglik(X, y, np.where(np.arange(len(W))[:, None] == 3, 0.0, W)) == -np.inf      # d_3 = 0
    three = np.stack([X[:100], const, X[100:200]])
    got = elfi_amd.wsemi_loglik(three, y, W)
    assert got[1] == -np.inf and np.isfinite(got[0]) and np.isfinite(got[2])
    assert got[0] == elfi_amd.wsemi_loglik(X[:100], y, W) and got[2] == elfi_amd.wsemi_loglik(X[100:200], y, W)
    out = np.zeros(1)
    for bad in (None, np.where(np.arange(W.size).reshape(W.shape) == 5, np.inf, W)):
        with pytest.raises(ValueError):          # ELFIHIP_ERR_ARG, before any launch
            hip_ctx.call("elfihip_wsemi_loglik", _lib.ptr(X), 1, len(X), X.shape[1], X.shape[1], _lib.ptr(y), _lib.ptr(bad),
                         None, 0, None, 0, _lib.ptr(out), None, None, None, None)


def test_device_pointer_form_at_a_pitch_and_an_offset_equals_the_host_form(hip_ctx):
    import elfi_amd
    import torch
    from elfi_amd import _lib
    X, y, W = R.make_case(4)
    n, m = X.shape
    G, ng, ldx = 2, n // 2, m + 3
    X, pre, pens = X[:G * ng], np.array([ng // 2 + 1, ng], dtype=np.int64), np.array([0.1, 0.6])
    want, wu, wrho, wd, wsc = elfi_amd.wsemi_loglik(X, y, W, n_groups=G, prefixes=pre, shrinkage='warton',
                                                    penalties=list(pens), return_parts=True)
    assert want.shape == (G, 2, 2) and np.all(np.isfinite(want))
    (keep, dX), (keep_y, dy), (keep_w, dW) = DL.place(X, ldx, 1), DL.place(y[None, :], m, 1), DL.place(W, m, 1)
    oll, ou, od = DL.guarded_out(G, 4, off=1), DL.guarded_out(G, m), DL.guarded_out(G, m, off=1)
    orho, osc = DL.guarded_out(G, m * m, off=1), DL.guarded_out(G * ng, m)
    torch.cuda.synchronize()
    hip_ctx.call("elfihip_wsemi_loglik_dev", dX, G, ng, m, ldx, dy, dW, _lib.ptr(pre), len(pre), _lib.ptr(pens), len(pens),
                 oll.ptr, ou.ptr, orho.ptr, od.ptr, osc.ptr)
    hip_ctx.synchronize()
    assert np.array_equal(oll.check().reshape(want.shape), want)
    assert np.array_equal(ou.check(), wu) and np.array_equal(orho.check().reshape(wrho.shape), wrho)
    assert np.array_equal(od.check(), wd) and np.array_equal(osc.check().reshape(wsc.shape), wsc)


class _Model:           # what the batched tools ask of a model: generate() hands out the groups made by hand, one per call
    parameter_names = ['t']

    def __init__(self, groups, y):
        self.groups, self.calls, self.y = groups, 0, y

    def __getitem__(self, name):
        return type('Node', (), dict(observed=self.y))

    def generate(self, n, outputs, with_values, seed):
        self.calls += 1
        return {'S': self.groups[self.calls - 1][:n]}


def test_likelihood_callable_and_the_batched_tools(hip_ctx):
    import elfi_amd
    X, y, W = R.make_case(2)
    lik = elfi_amd.whitened_semiparametric_likelihood(W, **WARTON)
    a = lik(X, y[None, :])
    assert isinstance(a, np.ndarray) and a.shape == (1,) and a[0] == elfi_amd.wsemi_loglik(X, y, W, **WARTON)
    rs = np.random.RandomState(11)
    groups = np.stack([X[rs.permutation(len(X))] + rs.randn(*X.shape) for _ in range(4)])
    counts, lmdas = [20, 33], [0.2, 0.4, 0.6]
    one = lambda g, p, lm: elfi_amd.wsemi_loglik(g[:p], y, W, shrinkage='warton', penalty=lm)
    single = np.array([[[one(g, p, lm) for lm in lmdas] for p in counts] for g in groups])
    lm, sd = elfi_amd.select_penalty(_Model(groups, y), counts, [0.0], 'S', likelihood=lik, lmdas=lmdas, M=4, sigma=1.0)
    spread = single.std(axis=0)
    pick = np.abs(spread - 1.0).argmin(axis=1)
    assert np.array_equal(lm, np.array(lmdas)[pick]) and np.array_equal(sd, spread[[0, 1], pick])
    std = elfi_amd.log_SL_stdev(_Model(groups, y), [0.0], counts, 'S', likelihood=lik, M=4)
    assert np.array_equal(std, np.std(np.ascontiguousarray(single[:, :, 1].T), axis=1))
