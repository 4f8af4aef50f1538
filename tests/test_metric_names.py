"""The distance path's metric-name table (elfi_amd/_lib.py) against SciPy's own alias table and the C header.  No GPU."""
import os
import re

import pytest
import scipy.spatial.distance as ssd

import elfi_amd
from elfi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEVEN = ('euclidean', 'sqeuclidean', 'cityblock', 'chebyshev', 'minkowski', 'seuclidean', 'mahalanobis',
          'canberra', 'braycurtis', 'cosine', 'correlation')


def test_table_is_scipys_alias_table():
    expected = {alias: name for name in ELEVEN for alias in ssd._METRICS[name].aka}
    assert {a: v[0] for a, v in _lib.METRIC_NAMES.items()} == expected
    assert set(_lib.METRICS) == set(ELEVEN)
    for alias, (name, mid) in _lib.METRIC_NAMES.items():
        assert mid == _lib.METRICS[name]


def test_ids_match_the_header():
    text = open(os.path.join(ROOT, 'include', 'elfihip.h')).read()
    ids = {k.lower(): int(v) for k, v in re.findall(r'ELFIHIP_([A-Z]+) = (\d+),?\s*/\*', text)
           if k.lower() in ELEVEN}
    assert ids == _lib.METRICS


def test_letter_case_and_unknown_names():
    for alias, (name, mid) in _lib.METRIC_NAMES.items():
        assert _lib.resolve_metric(alias.upper()) == (name, mid)
        assert _lib.resolve_metric(alias.capitalize()) == (name, mid)
    # every other name SciPy knows, and names it does not, are refused
    others = [n for n in ssd._METRICS if n not in ELEVEN]
    assert 'hamming' in others and 'jensenshannon' in others
    for name in others + [a for n in others for a in ssd._METRICS[n].aka] + ['nonsense', '', 'wminkowski', 'euclidean ']:
        with pytest.raises(ValueError):
            _lib.resolve_metric(name)
        with pytest.raises(ValueError):
            elfi_amd.HipDistance(name)
    with pytest.raises(ValueError):
        _lib.resolve_metric(None)


@pytest.mark.parametrize('name,canon', [('cos', 'cosine'), ('CO', 'correlation'), ('Canberra', 'canberra'),
                                        ('braycurtis', 'braycurtis'), ('mahal', 'mahalanobis'), ('EU', 'euclidean')])
def test_hip_distance_keeps_the_canonical_name(name, canon):
    kw = {'VI': [[1.0]]} if canon == 'mahalanobis' else {}
    assert elfi_amd.HipDistance(name, **kw).metric == canon
    assert repr(elfi_amd.HipDiscrepancy(name, **kw)) == 'HipDiscrepancy(%r)' % canon
