"""GPU: the summary-statistic selection kernels (csrc/twostage.hip) through the C ABI and the Python mirrors.

Yardstick (see tests/test_twostage.py): `truth`, the quantity in 40-digit arithmetic; the bound is 16 x the reference's
largest own error over the recorded cases with the same number of parameters, never below 16 eps (1 + |truth|).
The k-th distances are compared with the brute-force statement within (q + 4) ulps: each side carries at most (q + 2) eps
on the sum of squares, halved by the square root, plus half an ulp of its rounding.
Measured errors are printed per case (pytest -s).
"""
import ctypes as C
import os

import numpy as np
import pytest

import device_layout as L
import ref_shim
import twostage_ref as R

pytestmark = pytest.mark.gpu
needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')

ERR_ARG = 1


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'twostage.npz'))


def same_kth(got, want, q):
    """Equal where infinite or zero, else within (q + 4) ulps."""
    got, want = np.asarray(got), np.asarray(want)
    exact = ~np.isfinite(want) | (want == 0.0)
    return np.array_equal(got[exact], want[exact]) and np.all(R.ulps(got[~exact], want[~exact]) <= q + 4)


@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_yardstick_and_kth_distances(gold, ci):
    import elfi_amd
    T, Cl, k = R.make_case(ci)
    q = T.shape[1]
    E, kth = elfi_amd.knn_entropy(T, k=k, return_kth=True)
    M = elfi_amd.mrsse(T, Cl)
    assert isinstance(E, float) and isinstance(M, float) and kth.shape == (len(T),)
    want_kth = R.kth_distances_ref(T, k)[0]
    print('case %d n=%d q=%d k=%d  kth: %.2f ulps at most' % (ci, len(T), q, k, R.ulps(kth, want_kth).max()))
    assert same_kth(kth, want_kth, q)
    same = R.same_q(ci)
    for name, got in (('entropy', E), ('mrsse', M)):
        truth, e_ref = gold['truth_' + name][ci], gold['e_' + name]
        tol = R.bound(e_ref[same], truth)
        dev = abs(got - truth)
        print('case %d n=%d q=%d k=%d %-7s e_ref %.2e device %.2e bound %.2e' % (ci, len(T), q, k, name, e_ref[ci], dev, tol))
        assert dev <= tol, (name, dev, tol)


# n: one point, a few, around the tile of 256, a tile tail, several workgroups; q: every instance width; k: the list
# classes 4 / 8 / 16 and their boundary, k = n and k = n + 1
KNN_CASES = [(1, 1, 1), (1, 2, 2), (5, 2, 5), (5, 3, 6), (5, 8, 1), (5, 32, 4), (255, 1, 4), (255, 3, 16), (256, 2, 4),
             (256, 8, 5), (257, 2, 8), (257, 32, 16), (257, 3, 2), (513, 2, 4), (513, 1, 5), (513, 8, 16), (1200, 2, 4),
             (1200, 3, 8), (1200, 32, 5), (1200, 1, 1)]


def entropy_tolerance(want_kth, q, E):
    """Device against the statement, both from k-th distances that agree within (q + 4) ulps: a log is good to an ulp on
    either side (2 eps |log R|) and moves by (q + 4) eps with its argument; the device adds the n logs in a tree of depth 8
    and then n / 256 partials in a row ((9 + n / 256) eps sum |log R| at most; the statement's sum is exact); the constant
    and the last two operations are a few roundings of numbers of the size of E."""
    n = len(want_kth)
    logs = np.abs(np.log(want_kth))
    return (q / n) * R.EPS * ((2 + 9 + n / 256) * logs.sum() + n * (q + 4)) + 8 * R.EPS * (1 + abs(E))


@pytest.mark.parametrize('n,q,k', KNN_CASES)
def test_knn_cases(n, q, k):
    import elfi_amd
    rs = np.random.RandomState(1000 * n + 10 * q + k)
    T = 0.5 + 1.5 * rs.randn(n, q)
    E, kth = elfi_amd.knn_entropy(T, k=k, return_kth=True)
    want_kth = R.kth_distances_ref(T, k)[0]
    want = R.knn_entropy_ref(T, k)[0]
    assert same_kth(kth, want_kth, q)
    if k == 1:
        assert E == -np.inf and np.all(kth == 0.0)
    elif k > n:
        assert E == np.inf and np.all(np.isposinf(kth))
    else:
        tol = entropy_tolerance(want_kth, q, want)
        print('n=%d q=%d k=%d entropy % .15g device-statement %.2e tolerance %.2e' % (n, q, k, want, abs(E - want), tol))
        assert abs(E - want) <= tol


def test_coincident_points_do_not_disturb_the_neighbouring_groups():
    import elfi_amd
    rs = np.random.RandomState(5)
    G = rs.randn(3, 50, 2)
    G[1, 10:14] = G[1, 10]                     # 4 coincident points in the middle group: R_i4 = 0 for them
    E, kth = elfi_amd.knn_entropy(G, k=4, return_kth=True)
    assert E[1] == -np.inf and np.all(kth[1, 10:14] == 0.0) and np.all(kth[1, :10] > 0.0)
    for g in (0, 2):
        Eg, kg = elfi_amd.knn_entropy(G[g], k=4, return_kth=True)
        assert E[g] == Eg and np.isfinite(Eg) and np.array_equal(kth[g], kg)
    assert np.isfinite(elfi_amd.knn_entropy(G[1], k=5))


def test_same_sums_same_bits(hip_ctx):
    import elfi_amd
    import torch
    rs = np.random.RandomState(8)
    G, n, q, k, J = 7, 300, 2, 4, 9
    T = rs.randn(G, n, q) * np.linspace(0.2, 3.0, G)[:, None, None]
    Cl = rs.randn(J, q)
    E, kth = elfi_amd.knn_entropy(T, k=k, return_kth=True)
    M = elfi_amd.mrsse(T, Cl)
    assert E.shape == (G,) and kth.shape == (G, n) and M.shape == (G,)
    for g in range(G):                          # a group's result does not depend on G
        Eg, kg = elfi_amd.knn_entropy(T[g], k=k, return_kth=True)
        assert Eg == E[g] and np.array_equal(kg, kth[g]) and elfi_amd.mrsse(T[g], Cl) == M[g]
    flat = T.reshape(G * n, q)                  # the flat form
    Ef, kf = elfi_amd.knn_entropy(flat, k=k, n_groups=G, return_kth=True)
    assert np.array_equal(Ef, E) and np.array_equal(kf, kth) and np.array_equal(elfi_amd.mrsse(flat, Cl, n_groups=G), M)
    for pad, off in ((3, 1), (2, 0), (0, 0)):   # the _dev forms at the caller's pitch and alignment
        ldt = q + pad
        dT, pT = L.place(flat, ldt, off)
        dC, pC = L.place(Cl, ldt + 1, off)
        oE, oK, oM = L.guarded_out(G), L.guarded_out(G * n, 1, off), L.guarded_out(G, 1, off)
        torch.cuda.synchronize()
        hip_ctx.call("elfihip_knn_entropy_dev", pT, G, n, q, ldt, k, oE.ptr, oK.ptr)
        hip_ctx.call("elfihip_mrsse_dev", pT, G, n, q, ldt, pC, J, ldt + 1, oM.ptr)
        hip_ctx.synchronize()
        assert np.array_equal(oE.check(), E) and np.array_equal(oK.check().reshape(G, n), kth)
        assert np.array_equal(oM.check(), M)
    # without the optional output
    oE = L.guarded_out(G)
    dT, pT = L.place(flat, q, 0)
    torch.cuda.synchronize()
    hip_ctx.call("elfihip_knn_entropy_dev", pT, G, n, q, q, k, oE.ptr, None)
    hip_ctx.synchronize()
    assert np.array_equal(oE.check(), E)


def subset_case(n, m, C, seed):
    rs = np.random.RandomState(seed)
    X, y = rs.randn(n, m) * np.linspace(0.5, 2.0, m), rs.randn(m)
    if n > 11:
        X[7] = X[3]                  # two equal distances under every mask: the lower row comes first
        X[11, 0] = np.nan            # NaN under every mask (selected: NaN; unselected: 0 * NaN): the row comes last
    masks = (rs.rand(C, m) < 0.5).astype(np.float64)
    masks[np.arange(C), rs.randint(0, m, C)] = 1.0          # no all-zero mask
    return X, y, masks


def device_distances(X, y, masks):
    import elfi_amd
    return np.column_stack([elfi_amd.nested_weighted_euclidean(X, y, masks[c0:c0 + 64]) for c0 in range(0, len(masks), 64)])


# (n, m, C, k): k = 1, a usual k and k = n + 3 (clipped to n); C = 65 takes two blocks; k > 2048 takes the sort's global steps
SUBSET_CASES = [(1000, 2, 1, 1), (1000, 5, 15, 500), (1000, 64, 65, 1003), (70000, 5, 15, 500), (70000, 2, 65, 1),
                (70000, 64, 1, 70003), (1000, 5, 65, 500)]


@pytest.mark.parametrize('n,m,C,k', SUBSET_CASES)
def test_subset_best(n, m, C, k):
    import elfi_amd
    X, y, masks = subset_case(n, m, C, seed=n + m + C)
    vals, rows = elfi_amd.subset_best(X, y, masks, k)
    D = device_distances(X, y, masks)
    want_vals, want_rows = R.best_of_columns(D, k)
    assert vals.shape == rows.shape == (C, min(k, n)) and rows.dtype == np.int64
    assert np.array_equal(rows, want_rows)
    assert np.array_equal(vals.view(np.int64), np.ascontiguousarray(want_vals).view(np.int64))     # bit for bit, NaN included
    if k >= n:
        assert np.all(rows[:, -1] == 11) and np.all(np.isnan(vals[:, -1]))
        where3 = np.argmax(rows == 3, axis=1)
        assert np.all(rows[np.arange(C), where3 + 1] == 7) and np.all(vals[np.arange(C), where3] == vals[np.arange(C), where3 + 1])
    # the statement on the host sums the selected columns alone: the same numbers
    few = slice(0, min(C, 3))
    assert np.array_equal(R.subset_distances(X[:500], y, masks[few])[:10], D[:10, few])


def test_subset_best_dev_at_the_callers_pitch(hip_ctx):
    import elfi_amd
    import torch
    n, m, C, k = 3000, 5, 15, 500
    X, y, masks = subset_case(n, m, C, seed=77)
    vals, rows = elfi_amd.subset_best(X, y, masks, k)
    for pad, off in ((3, 1), (1, 0), (0, 0)):
        dX, pX = L.place(X, m + pad, off)
        dy = L.to_device(y)
        oV = L.guarded_out(C, k, off)
        dR = torch.full((2 + C * k + 8,), -77, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        hip_ctx.call("elfihip_subset_best_dev", pX, n, m, m + pad, dy.data_ptr(), masks.ctypes.data, C, k, oV.ptr,
                     dR.data_ptr() + 16)
        hip_ctx.synchronize()
        assert np.array_equal(oV.check().view(np.int64), vals.view(np.int64))
        hR = dR.cpu().numpy()
        assert np.all(hR[:2] == -77) and np.all(hR[2 + C * k:] == -77) and np.array_equal(hR[2:2 + C * k].reshape(C, k), rows)


def test_c_entry_points_refuse_bad_arguments_with_outputs_untouched(hip_ctx):
    rs = np.random.RandomState(2)
    T = np.ascontiguousarray(rs.randn(40, 33))
    out = np.full(64, L.SENTINEL)
    rows = np.full(64, -77, dtype=np.int64)
    lib, h = hip_ctx.lib, hip_ctx.handle
    p = lambda a: C.c_void_p(a.ctypes.data)      # noqa: E731
    knn = [dict(q=33), dict(k=0), dict(k=17), dict(n=0), dict(ldt=2)]
    for kw in knn:
        a = dict(G=1, n=10, q=3, ldt=3, k=4)
        a.update(kw)
        for name in ("elfihip_knn_entropy", "elfihip_knn_entropy_dev"):
            rc = getattr(lib, name)(h, p(T), a['G'], a['n'], a['q'], a['ldt'], a['k'], p(out), p(out[8:]))
            assert rc == ERR_ARG and lib.elfihip_last_error(h), (name, kw)
    for kw in (dict(q=33), dict(n=0), dict(ldt=2), dict(ldc=2), dict(J=0)):
        a = dict(G=1, n=10, q=3, ldt=3, J=4, ldc=3)
        a.update(kw)
        for name in ("elfihip_mrsse", "elfihip_mrsse_dev"):
            rc = getattr(lib, name)(h, p(T), a['G'], a['n'], a['q'], a['ldt'], p(T), a['J'], a['ldc'], p(out))
            assert rc == ERR_ARG, (name, kw)
    good = np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    half, zero = good.copy(), good.copy()
    half[1, 1] = 0.5
    zero[1] = 0.0
    for masks, kw in ((half, {}), (zero, {}), (good, dict(n=0)), (good, dict(ldx=2)), (good, dict(k=0))):
        a = dict(n=10, m=3, ldx=3, k=4)
        a.update(kw)
        for name in ("elfihip_subset_best", "elfihip_subset_best_dev"):
            rc = getattr(lib, name)(h, p(T), a['n'], a['m'], a['ldx'], p(T), p(masks), 2, a['k'], p(out), p(rows))
            assert rc == ERR_ARG, (name, kw)
    hip_ctx.synchronize()
    assert np.all(out.view(np.int64) == np.float64(L.SENTINEL).view(np.int64)) and np.all(rows == -77)


@needs_reference
def test_end_to_end_against_the_reference_run(gold):
    import elfi_amd
    elfi = ref_shim.install()
    from elfi.methods.diagnostics import TwoStageSelection
    run = R.MA2_RUN
    cands = R.ma2_candidates()
    sel = elfi_amd.HipTwoStageSelection(R.ma2_simulator(elfi), 'euclidean', list_ss=cands, seed=run['seed'])
    assert isinstance(sel, TwoStageSelection)
    chosen = sel.run(run['n_sim'], run['n_acc'], run['n_closest'], batch_size=run['batch_size'], k=run['k'])
    assert tuple(f.__name__ for f in chosen) == tuple(gold['ma2_chosen']) == ('ac1', 'ac2', 'var')
    assert all(any(f is c for c in cands) for f in chosen)
    assert tuple(sel.names_min_entropy_) == tuple(gold['ma2_min_entropy'])
    combos = R.combination_names()
    for c in R.MA2_RECORDED:
        assert np.array_equal(sel.accepted_[combos.index(c)], gold['ma2_accepted_' + '_'.join(c)])
    same = [i for i, c in enumerate(R.CASES) if c[2] == 2]
    for name, got in (('entropy', sel.entropies_), ('mrsse', sel.mrsses_)):
        e_ref = gold['e_' + name][same]
        for ci, c in enumerate(combos):
            ref = gold['ma2_' + name][ci]
            tol = R.bound(e_ref, ref) + e_ref.max()
            print('%-24s %-7s reference % .15g device-reference %.2e tolerance %.2e' % (','.join(c), name, ref, abs(got[ci] - ref), tol))
            assert abs(got[ci] - ref) <= tol
