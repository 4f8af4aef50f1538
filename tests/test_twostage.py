"""CPU: the NumPy/SciPy statement of the summary-statistic selection's quantities (tests/twostage_ref.py) against the
values recorded from the reference's TwoStageSelection (tests/golden/twostage.npz, scripts/make_golden_twostage.py), the
argument handling of the Python mirrors (elfi_amd/twostage.py), which happens before any device call, and -- where the
reference package is present -- the one-pass plumbing of HipTwoStageSelection with the three device calls replaced by
the statement.

Tolerance: the yardstick is `truth` (the quantity in 40-digit arithmetic on the same float inputs).  A value must lie
within 16 x max(e_ref over the recorded cases with the same number of parameters q), e_ref = |reference - truth|, and the
bound is never below 16 eps (1 + |truth|) (twostage_ref.bound).
"""
import os

import numpy as np
import pytest

import ref_shim
import twostage_ref as R

needs_reference = pytest.mark.skipif(not ref_shim.available(), reason='no reference package (run oracle/make_ref.sh)')


@pytest.fixture(scope='module')
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, 'twostage.npz'))


def test_fixture_matches_the_recipe(gold):
    assert np.array_equal(gold['cases'], np.array(R.CASES, dtype=float))
    assert {c[2] for c in R.CASES} == {1, 2, 3, 8, 32}
    for key in ('ref_entropy', 'ref_mrsse', 'truth_entropy', 'truth_mrsse', 'e_entropy', 'e_mrsse'):
        assert gold[key].shape == (len(R.CASES),) and np.all(np.isfinite(gold[key]))
    assert np.all(gold['e_entropy'] < 1e-12) and np.all(gold['e_mrsse'] < 1e-12)
    combos = [tuple(s.split(',')) for s in gold['ma2_combinations']]
    assert combos == R.combination_names() and len(combos) == 15
    assert gold['ma2_entropy'].shape == gold['ma2_mrsse'].shape == (15,)
    assert tuple(gold['ma2_min_entropy']) == combos[int(np.argmin(gold['ma2_entropy']))]
    assert tuple(gold['ma2_chosen']) == combos[int(np.argmin(gold['ma2_mrsse']))]
    for c in R.MA2_RECORDED:
        assert gold['ma2_accepted_' + '_'.join(c)].shape == (R.MA2_RUN['n_acc'], 2)


@pytest.mark.parametrize('ci', range(len(R.CASES)))
def test_restatement_against_truth_and_reference(gold, ci):
    T, Cl, k = R.make_case(ci)
    same = R.same_q(ci)
    for name, got in (('entropy', R.knn_entropy_ref(T, k)[0]), ('mrsse', R.mrsse_ref(T, Cl)[0])):
        truth, e_ref = gold['truth_' + name][ci], gold['e_' + name]
        tol = R.bound(e_ref[same], truth)
        dev = abs(got - truth)
        print('case %d n=%d q=%d k=%d %-7s e_ref %.2e restatement %.2e bound %.2e'
              % (ci, len(T), T.shape[1], k, name, e_ref[ci], dev, tol))
        assert dev <= tol, (name, dev, tol)
        assert abs(got - gold['ref_' + name][ci]) <= tol + e_ref[ci]


def test_restatement_neighbour_rules_and_groups():
    T, Cl, k = R.make_case(1)
    # the point itself is the first neighbour: k = 1 is distance 0, k > n is inf
    assert np.all(R.kth_distances_ref(T, 1) == 0.0) and R.knn_entropy_ref(T, 1)[0] == -np.inf
    assert R.knn_entropy_ref(T[:5], 6)[0] == np.inf and np.all(np.isinf(R.kth_distances_ref(T[:5], 6)))
    # against a plain per-point sort
    i = 17
    d = np.sort(np.sqrt(((T - T[i]) ** 2).sum(axis=1)))
    assert R.ulps(R.kth_distances_ref(T, 4)[0, i], d[3]) <= 2
    # k coincident points
    Tc = T[:50].copy()
    Tc[10:14] = Tc[10]
    assert R.knn_entropy_ref(Tc, 4)[0] == -np.inf and np.isfinite(R.knn_entropy_ref(Tc, 5)[0])
    # groups: each as its own call
    two = R.knn_entropy_ref(T, 4, n_groups=2)
    assert two[0] == R.knn_entropy_ref(T[:250], 4)[0] and two[1] == R.knn_entropy_ref(T[250:], 4)[0]
    m2 = R.mrsse_ref(T, Cl, n_groups=2)
    assert m2[1] == R.mrsse_ref(T[250:], Cl)[0]


def test_restatement_subset_best():
    rs = np.random.RandomState(3)
    X, y = rs.randn(200, 4), rs.randn(4)
    X[7] = X[3]                      # two equal distances: the lower row first
    X[11, 2] = np.nan                # NaN in column 2: last wherever the mask selects (or multiplies) it
    masks = np.array([[1, 1, 0, 0], [0, 0, 1, 0], [1, 1, 1, 1.0]])
    vals, rows = R.subset_best_ref(X, y, masks, 200)
    D = R.subset_distances(X, y, masks)
    np.testing.assert_array_equal(D[:, 0], np.sqrt((X[:, 0] - y[0]) ** 2 + (X[:, 1] - y[1]) ** 2))
    assert list(rows[0]).index(3) + 1 == list(rows[0]).index(7)
    assert rows[1, -1] == 11 and np.isnan(vals[1, -1]) and rows[2, -1] == 11
    assert np.all(np.diff(vals[0]) >= 0)
    v3, r3 = R.subset_best_ref(X, y, masks, 203)
    assert v3.shape == (3, 200)


def test_argument_errors_come_before_any_device_call(monkeypatch):
    import elfi_amd
    from elfi_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('a device context was asked for')
    monkeypatch.setattr(_lib, 'default_context', no_device)
    rs = np.random.RandomState(0)
    T = rs.randn(40, 3)
    for kw in (dict(k=0), dict(k=17), dict(k=2.5), dict(n_groups=3), dict(n_groups=0)):
        with pytest.raises(ValueError):
            elfi_amd.knn_entropy(T, **kw)
    with pytest.raises(ValueError):
        elfi_amd.knn_entropy(rs.randn(40, 33))                      # q = 33
    with pytest.raises(ValueError):
        elfi_amd.knn_entropy(np.empty((0, 3)))                      # n = 0
    with pytest.raises(ValueError):
        elfi_amd.knn_entropy(rs.randn(2, 10, 3), n_groups=3)
    with pytest.raises(ValueError):
        elfi_amd.knn_entropy(rs.randn(40))
    with pytest.raises(ValueError):
        elfi_amd.mrsse(T, rs.randn(5, 2))
    with pytest.raises(ValueError):
        elfi_amd.mrsse(T, np.empty((0, 3)))
    with pytest.raises(ValueError):
        elfi_amd.mrsse(rs.randn(40, 33), rs.randn(5, 33))
    X, y = rs.randn(30, 4), rs.randn(4)
    ok = np.array([[1, 0, 1, 0.0]])
    for args in ((X, y, [[1, 0.5, 0, 0]], 5), (X, y, [[1, 0, 0, 0], [0, 0, 0, 0]], 5), (X, y, ok, 0), (X, y[:3], ok, 5),
                 (X, y, [[1, 0, 1]], 5), (np.empty((0, 4)), y, ok, 5), (X, y, [[1, 0, np.nan, 0]], 5)):
        with pytest.raises(ValueError):
            elfi_amd.subset_best(*args)
    # the metric is checked before the reference's class is even looked for
    for bad in ('cityblock', 'Euclidean', lambda *a: 0.0):
        with pytest.raises(NotImplementedError, match='euclidean'):
            elfi_amd.HipTwoStageSelection(None, bad, list_ss=[np.mean])


def test_candidate_layout():
    from elfi_amd import twostage
    a, b, c = (lambda x: x), (lambda x: x), (lambda x: x)
    distinct, index = twostage._candidate_layout([(a,), (b,), (a, b), (b, c), (a, b, c)])
    assert distinct == [a, b, c] and index == [[0], [1], [0, 1], [1, 2], [0, 1, 2]]
    with pytest.raises(NotImplementedError):
        twostage._candidate_layout([(a, b), (b, a)])
    with pytest.raises(NotImplementedError):
        twostage._candidate_layout([(a, a)])


@needs_reference
def test_factories_have_the_reference_shapes():
    import elfi_amd
    elfi = ref_shim.install()
    from elfi.methods.diagnostics import TwoStageSelection
    cls = elfi_amd.hip_two_stage_selection_class()
    assert cls is elfi_amd.hip_two_stage_selection_class() and issubclass(cls, TwoStageSelection)
    assert cls.__init__ is TwoStageSelection.__init__ and cls._combine_ss is TwoStageSelection._combine_ss
    cands = R.ma2_candidates()
    sel = elfi_amd.HipTwoStageSelection(R.ma2_simulator(elfi), 'euclidean', list_ss=cands, max_cardinality=2, seed=3)
    assert isinstance(sel, TwoStageSelection) and sel.seed == 3 and len(sel.ss_candidates) == 4 + 6
    with pytest.raises(ValueError, match='too small'):
        sel.run(100, 200)
    with pytest.raises(ValueError, match='too small'):
        sel.run(1000)                                    # n_closest = int(10 / 100) = 0, the reference's default
    with pytest.raises(ValueError):
        elfi_amd.HipTwoStageSelection(R.ma2_simulator(elfi), 'euclidean')
    sel.fn_distance = 'cityblock'
    with pytest.raises(NotImplementedError):
        sel.run(1000, 100, 10)


@needs_reference
def test_one_pass_plumbing_reproduces_the_reference_run(gold, monkeypatch, caplog):
    """HipTwoStageSelection.run with the three device calls replaced by the statement: the single simulation pass, the
    masks and the gathering give the reference's accepted parameters exactly, and its choice."""
    import logging
    import elfi_amd
    from elfi_amd import twostage
    elfi = ref_shim.install()
    monkeypatch.setattr(twostage, 'subset_best', lambda X, y, masks, k, ctx=None: R.subset_best_ref(X, y, masks, k))
    monkeypatch.setattr(twostage, 'knn_entropy', lambda T, k=4, **kw: R.knn_entropy_ref(T, k))
    monkeypatch.setattr(twostage, 'mrsse', lambda T, Cl, **kw: R.mrsse_ref(T, Cl))
    run = R.MA2_RUN
    cands = R.ma2_candidates()
    sel = elfi_amd.HipTwoStageSelection(R.ma2_simulator(elfi), 'euclidean', list_ss=cands, seed=run['seed'])
    with caplog.at_level(logging.INFO, logger='elfi_amd.twostage'):
        chosen = sel.run(run['n_sim'], run['n_acc'], run['n_closest'], batch_size=run['batch_size'], k=run['k'])
    assert tuple(f.__name__ for f in chosen) == tuple(gold['ma2_chosen']) and all(f in cands for f in chosen)
    assert tuple(sel.names_min_entropy_) == tuple(gold['ma2_min_entropy'])
    combos = R.combination_names()
    for c in R.MA2_RECORDED:
        np.testing.assert_array_equal(sel.accepted_[combos.index(c)], gold['ma2_accepted_' + '_'.join(c)])
    same = [i for i, c in enumerate(R.CASES) if c[2] == 2]
    for name, got in (('entropy', sel.entropies_), ('mrsse', sel.mrsses_)):
        for ci in range(15):
            ref = gold['ma2_' + name][ci]
            e_ref = gold['e_' + name][same]
            assert abs(got[ci] - ref) <= R.bound(e_ref, ref) + e_ref.max()     # bound + the reference's own error
    text = caplog.text
    assert "Combination ['ac1', 'ac2'] shows the entropy of -1.008348" in text
    assert "The minimum MRSSE of 7.932928 was found in ['ac1', 'ac2', 'var']." in text
