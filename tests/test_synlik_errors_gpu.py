"""GPU (a context is needed, no kernel is launched): the status and the elfihip_last_error text of invalid calls of the six
C entry points of the synthetic likelihoods -- elfihip_syn_loglik, elfihip_semi_loglik and elfihip_wsemi_loglik, each with
and without _dev -- at G = 1, n = 4, m = 2.  The texts were recorded from the library as it stood before the host side of
these entry points was written once; Python raises them as ValueError, so they stay character for character.  Every call
fails its checks before a pointer is read, so host arrays stand in for the device pointers of the _dev forms.
"""
import numpy as np
import pytest

from elfi_amd._lib import ERR_ARG

pytestmark = pytest.mark.gpu

SYN, SEMI, WSEMI = 'synthetic likelihood', 'semiparametric likelihood', 'whitened semiparametric likelihood'
ENTRY = {SYN: 'elfihip_syn_loglik', SEMI: 'elfihip_semi_loglik', WSEMI: 'elfihip_wsemi_loglik'}
SUMMARIES = '%s: %d summaries; 1 to 64 are supported'
ROWS = '%s: %d rows per group; 2 to 16384 are supported'

# (changed arguments, the text; %s: the likelihood's name) for all three
COMMON = [
    (dict(m=0), SUMMARIES % ('%s', 0)),
    (dict(m=65, ldx=65), SUMMARIES % ('%s', 65)),
    (dict(ldx=1), 'bad shape G=1 n=4 m=2 ldx=1'),
    (dict(y=None), 'NULL data pointer'),
    (dict(K=2), 'prefixes and K do not agree (K=2)'),
    (dict(prefixes=[2, 4], K=0), 'prefixes and K do not agree (K=0)'),
    (dict(prefixes=[4, 2], K=2), 'prefixes must be ascending and at least 2 (entry 1)'),
    (dict(prefixes=[2, 3], K=2), 'the last prefix must be n'),
    (dict(penalties=[1.5], P=1), 'penalty 0 is outside [0, 1]'),
]
OWN = {
    SYN: [(dict(n=1), 'bad shape G=1 n=1 m=2 ldx=2')],
    SEMI: [(dict(n=1), ROWS % (SEMI, 1)), (dict(n=16385), ROWS % (SEMI, 16385))],
    WSEMI: [(dict(n=1), ROWS % (WSEMI, 1)), (dict(n=16385), ROWS % (WSEMI, 16385)), (dict(W=None), 'the whitening matrix is NULL')],
}
CASES = [(what, kw, text % what if '%s' in text else text) for what in ENTRY for kw, text in COMMON + OWN[what]]


@pytest.mark.parametrize('what, kw, text', CASES, ids=['%s-%d' % (ENTRY[c[0]][8:], i) for i, c in enumerate(CASES)])
def test_invalid_call_leaves_the_recorded_status_and_text(hip_ctx, what, kw, text):
    X, y, W, out = np.zeros((4, 2)), np.zeros(2), np.eye(2), np.zeros(64)
    a = dict(n=4, m=2, ldx=2, y=y, W=W, prefixes=None, K=0, penalties=None, P=0)
    a.update(kw)
    p = lambda v: None if v is None else v.ctypes.data      # noqa: E731
    pre = None if a['prefixes'] is None else np.array(a['prefixes'], dtype=np.int64)
    pen = None if a['penalties'] is None else np.array(a['penalties'], dtype=np.float64)
    head = [p(X), 1, a['n'], a['m'], a['ldx'], p(a['y'])]
    lists = [p(pre), a['K'], p(pen), a['P'], p(out)]
    args = {SYN: head + [p(a['W']), 0, None] + lists + [None, None],
            SEMI: head + lists + [None, None, None],
            WSEMI: head + [p(a['W'])] + lists + [None, None, None, None]}[what]
    for name in (ENTRY[what], ENTRY[what] + '_dev'):
        assert getattr(hip_ctx.lib, name)(hip_ctx.handle, *args) == ERR_ARG, name
        assert hip_ctx.lib.elfihip_last_error(hip_ctx.handle).decode() == text, name
    assert not out.any()
