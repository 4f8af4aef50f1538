"""The sampler state's push policy (elfi_amd/csrc/reject_policy.hpp): route, merge interval and sizes.

The header is plain C++ (no HIP), so it is compiled here with g++ behind a tiny test-only C wrapper
(tests/cpp/reject_policy_capi.cpp) and needs no GPU.  Every expected value below is worked out by hand from the
formulas the sampler state has always used:
  full     = rows entered >= k
  expect   = n k / max(rows seen before this push, 1) for a full state, "infinite" otherwise
  route    = with an acceptance threshold: accept-and-select if device state, n >= 2^15 and expect > 8192, else filter;
             without: filter if expect <= 8192, else provisional if the caller can run a prefix pass, the state is not
             full, n >= 2^20 and 64 k <= n, else select
  interval = clamp(armed_pushes // (3 if sealing else 2), 1, 8); 1 for host-merge states and states not yet full
  s        = min(max(n // 16, 16384), n // 2);  mu = k s / n;  j = min(k, ceil(mu + 5 sqrt(mu) + 4))
  c_hi     = min(max(65536, 64 j), cap)
  list     = max(65536, 8 n)
"""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ACCEPT_SELECT, SELECT, PROVISIONAL, FILTER = range(4)
LL = C.c_longlong


@pytest.fixture(scope='module')
def rp(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('reject_policy') / 'libreject_policy_test.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-o', out,
                           os.path.join(HERE, 'cpp', 'reject_policy_capi.cpp')])
    lib = C.CDLL(out)
    lib.rp_route.restype = C.c_int
    lib.rp_route.argtypes = [LL, LL, LL, C.c_int, C.c_int, LL, C.c_int]
    lib.rp_interval.restype = LL
    lib.rp_interval.argtypes = [LL, C.c_int, C.c_int, C.c_int]
    lib.rp_provisional.restype = None
    lib.rp_provisional.argtypes = [LL, LL, LL, C.POINTER(LL)]
    lib.rp_list_size.restype = LL
    lib.rp_list_size.argtypes = [LL]
    return lib


def route(rp, n, k=1000, entered=0, rows_seen=0, host=False, accept=False, can_prefix=True):
    return rp.rp_route(k, entered, rows_seen, int(host), int(accept), n, int(can_prefix))


def test_header_is_plain_cxx():
    src = open(os.path.join(HERE, '..', 'elfi_amd', 'csrc', 'reject_policy.hpp')).read()
    assert 'hip_runtime' not in src and 'internal.hpp' not in src and 'elfihip_reject' not in src


@pytest.mark.parametrize('n, k, can_prefix, want', [
    (1000, 1000, True, SELECT),
    (1 << 20, 1000, True, PROVISIONAL),
    (1 << 20, 1000, False, SELECT),            # only a caller that can run a prefix pass is offered the route
    ((1 << 20) - 1, 1000, True, SELECT),
    (1 << 20, 16385, True, SELECT),            # 64 k = 1048640 > n
    (1 << 20, 16384, True, PROVISIONAL),       # 64 k = n
])
def test_route_state_not_full(rp, n, k, can_prefix, want):
    assert route(rp, n, k=k, can_prefix=can_prefix) == want
    assert route(rp, n, k=k, entered=k - 1, rows_seen=k - 1, can_prefix=can_prefix) == want


@pytest.mark.parametrize('n, host, want', [
    (32768, False, ACCEPT_SELECT),
    (32767, False, FILTER),
    (32768, True, FILTER),                     # a host-merge state never masks and selects
])
def test_route_with_acceptance_threshold(rp, n, host, want):
    assert route(rp, n, accept=True, host=host) == want
    assert route(rp, n, accept=True, host=host, can_prefix=False) == want


@pytest.mark.parametrize('rows_seen, n, want', [
    (10 ** 6, 10 ** 6, FILTER),                # expect = 1000
    (100, 1000, SELECT),                       # expect = 10^4 > 8192
    (1000, 8192, FILTER),                      # expect = 8192 exactly: the comparison is strict
    (1000, 8193, SELECT),
    (1 << 20, 1 << 24, SELECT),                # expect = 16000: a full state never takes the provisional route
])
def test_route_state_full(rp, rows_seen, n, want):
    assert route(rp, n, entered=1000, rows_seen=rows_seen) == want
    # with an acceptance threshold the same expectation picks accept-and-select (n >= 2^15, device state) or filter
    want_acc = ACCEPT_SELECT if want == SELECT and n >= 32768 else FILTER
    assert route(rp, n, entered=1000, rows_seen=rows_seen, accept=True) == want_acc


def test_interval_not_sealing(rp):
    got = [rp.rp_interval(p, 0, 0, 1) for p in (1, 2, 3, 4, 16, 17, 100)]
    assert got == [1, 1, 1, 2, 8, 8, 8]


def test_interval_sealing(rp):
    got = [rp.rp_interval(p, 1, 0, 1) for p in (1, 3, 6, 24, 25)]
    assert got == [1, 1, 2, 8, 8]


@pytest.mark.parametrize('seals', [0, 1])
@pytest.mark.parametrize('host, full', [(1, 1), (0, 0), (1, 0)])
def test_interval_forced(rp, seals, host, full):
    assert [rp.rp_interval(p, seals, host, full) for p in (1, 7, 24, 1000)] == [1, 1, 1, 1]


@pytest.mark.parametrize('n, k, cap, want', [
    (1 << 20, 1000, 8 << 20, (65536, 107, 65536)),        # mu = 62.5: 62.5 + 5 * 7.906 + 4 = 106.03
    (10 ** 7, 1000, 8 * 10 ** 7, (625000, 107, 65536)),   # the same mu
    (1 << 20, 16384, 8 << 20, (65536, 1188, 76032)),      # mu = 1024: 1024 + 160 + 4; 64 j = 76032
    (1 << 20, 16384, 70000, (65536, 1188, 70000)),
    (20000, 1000, 65536, (10000, 616, 65536)),            # below the route's minimum, formula only: s = n / 2; mu = 500
    (1 << 20, 5, 8 << 20, (65536, 5, 65536)),             # mu = 0.3125: 0.31 + 2.80 + 4 = 7.1 -> 8, capped at k
])
def test_provisional_sizes(rp, n, k, cap, want):
    out = (LL * 3)()
    rp.rp_provisional(n, k, cap, out)
    assert tuple(out) == want


def test_list_size(rp):
    assert rp.rp_list_size(100) == 65536
    assert rp.rp_list_size(10 ** 6) == 8 * 10 ** 6
