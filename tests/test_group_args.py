"""What the group-statistic entry points settle on the host (elfi_amd/csrc/group_args.hpp): the check of the prefix and
penalty lists, the parameter block and the tile count.

The header is plain C++ (no HIP), so it is compiled here with g++ behind a tiny test-only C wrapper
(tests/cpp/group_args_capi.cpp) and needs no GPU.  Every expected value below is worked out by hand:
  lists    prefixes go with K >= 1, no prefixes with K <= 1; penalties go with P >= 1, no penalties with P == 0;
           prefixes ascend strictly from at least 2 and end at n; 0 <= penalty <= 1 (a NaN is neither)
  errors   the first of these that fails, in that order, with the index of the offending entry
  block    [Ke prefixes as int64 bit patterns][Ke constants, only if given][P penalties]; Ke = K, or 1 without prefixes
           (the one prefix is n)
  tiles    ceil(m / 16)
"""
import ctypes as C
import os
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LL = C.c_longlong
N = 8    # rows per group in the list cases


@pytest.fixture(scope='module')
def ga(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('group_args') / 'libgroup_args_test.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-o', out,
                           os.path.join(HERE, 'cpp', 'group_args_capi.cpp')])
    lib = C.CDLL(out)
    lib.ga_tiles.restype = C.c_int
    lib.ga_tiles.argtypes = [C.c_int]
    lib.ga_lists_error.restype = C.c_int
    lib.ga_lists_error.argtypes = [C.POINTER(LL), C.c_int, C.POINTER(C.c_double), C.c_int, LL, C.c_char_p, C.c_int]
    lib.ga_params.restype = C.c_int
    lib.ga_params.argtypes = [C.POINTER(LL), C.c_int, LL, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int,
                              C.POINTER(C.c_double), C.c_int, C.POINTER(LL)]
    return lib


def _ll(v):
    return None if v is None else (LL * len(v))(*v)


def _dbl(v):
    return None if v is None else (C.c_double * len(v))(*v)


def lists_error(ga, prefixes, K, penalties, P, n=N):
    buf = C.create_string_buffer(128)
    length = ga.ga_lists_error(_ll(prefixes), K, _dbl(penalties), P, n, buf, len(buf))
    text = buf.value.decode()
    assert length == len(text)
    return text


def params(ga, prefixes, K, n, konst, penalties, P):
    """(Ke, offset of the constants, offset of the penalties, the block as a list of 8-byte words)"""
    words, out3 = (C.c_double * 16)(), (LL * 3)()
    length = ga.ga_params(_ll(prefixes), K, n, _dbl(konst), _dbl(penalties), P, words, len(words), out3)
    raw = bytes(words)[:8 * length]
    return out3[0], out3[1], out3[2], [raw[8 * i:8 * i + 8] for i in range(length)]


def as_int64(word):
    return struct.unpack('<q', word)[0]


def as_double(word):
    return struct.unpack('<d', word)[0]


def test_header_is_plain_cxx():
    src = open(os.path.join(HERE, '..', 'elfi_amd', 'csrc', 'group_args.hpp')).read()
    assert 'hip_runtime' not in src and 'common.hpp' not in src and 'internal.hpp' not in src


@pytest.mark.parametrize('prefixes, K, penalties, P, Ke', [
    (None, 0, None, 0, 1),                     # no lists: one prefix, the whole group
    (None, 1, None, 0, 1),                     # K = 1 without a list says the same
    ([2, 5, N], 3, None, 0, 3),                # prefixes only
    (None, 0, [0.25, 0.5], 2, 1),              # penalties only
    ([4, N], 2, [0.1, 0.2, 0.3], 3, 2),        # both
    ([N], 1, None, 0, 1),                      # K = 1 with prefixes = [n]
    (None, 0, [0.0], 1, 1),                    # the ends of [0, 1] are inside
    (None, 0, [1.0], 1, 1),
    (None, 0, [0.0, 1.0], 2, 1),
])
def test_accepted_lists(ga, prefixes, K, penalties, P, Ke):
    assert lists_error(ga, prefixes, K, penalties, P) == ''
    got_ke, konst, pen, words = params(ga, prefixes, K, N, None, penalties, P)
    assert got_ke == Ke and konst == Ke and pen == Ke
    assert len(words) - pen == P
    assert [as_int64(w) for w in words[:Ke]] == (prefixes or [N])
    assert [as_double(w) for w in words[pen:]] == (penalties or [])


ONE_ULP_ABOVE_ONE = 1.0 + 2.0 ** -52


@pytest.mark.parametrize('prefixes, K, penalties, P, text', [
    ([4, N], 0, None, 0, 'prefixes and K do not agree (K=0)'),
    (None, 2, None, 0, 'prefixes and K do not agree (K=2)'),
    (None, 0, None, 1, 'penalties and P do not agree (P=1)'),
    (None, 0, [0.5], 0, 'penalties and P do not agree (P=0)'),
    ([1, N], 2, None, 0, 'prefixes must be ascending and at least 2 (entry 0)'),
    ([4, 4, N], 3, None, 0, 'prefixes must be ascending and at least 2 (entry 1)'),
    ([8, 4], 2, None, 0, 'prefixes must be ascending and at least 2 (entry 1)'),
    ([4, N - 1], 2, None, 0, 'the last prefix must be n'),
    (None, 0, [0.5, -1e-300], 2, 'penalty 1 is outside [0, 1]'),
    (None, 0, [ONE_ULP_ABOVE_ONE], 1, 'penalty 0 is outside [0, 1]'),
    (None, 0, [0.0, 1.0, float('nan')], 3, 'penalty 2 is outside [0, 1]'),
])
def test_refused_lists(ga, prefixes, K, penalties, P, text):
    assert ONE_ULP_ABOVE_ONE > 1.0
    assert lists_error(ga, prefixes, K, penalties, P) == text


def test_errors_come_in_the_order_of_the_checks(ga):
    # everything wrong at once: K, then P, then the prefixes' order, then the last prefix, then the penalties
    assert lists_error(ga, [8, 4], 0, [1.5], 0) == 'prefixes and K do not agree (K=0)'
    assert lists_error(ga, [8, 4], 2, [1.5], 0) == 'penalties and P do not agree (P=0)'
    assert lists_error(ga, [8, 4], 2, [1.5], 1) == 'prefixes must be ascending and at least 2 (entry 1)'
    assert lists_error(ga, [4, 7], 2, [1.5], 1) == 'the last prefix must be n'
    assert lists_error(ga, [4, 8], 2, [1.5], 1) == 'penalty 0 is outside [0, 1]'


def test_block_with_constants(ga):
    c0, c1 = -12.5, 3.0625
    Ke, konst, pen, words = params(ga, [4, 8], 2, 8, [c0, c1], [0.25, 0.5], 2)
    assert (Ke, konst, pen) == (2, 2, 4)
    assert len(words) == 6
    assert [as_int64(w) for w in words[:2]] == [4, 8]
    assert [as_double(w) for w in words[2:]] == [c0, c1, 0.25, 0.5]


def test_block_without_constants(ga):
    Ke, konst, pen, words = params(ga, [4, 8], 2, 8, None, [0.25, 0.5], 2)
    assert (Ke, konst, pen) == (2, 2, 2)
    assert len(words) == 4
    assert [as_int64(w) for w in words[:2]] == [4, 8]
    assert [as_double(w) for w in words[2:]] == [0.25, 0.5]


def test_block_without_lists_is_the_one_prefix_n(ga):
    Ke, konst, pen, words = params(ga, None, 0, 7, None, None, 0)
    assert (Ke, konst, pen) == (1, 1, 1)
    assert [as_int64(w) for w in words] == [7]
    # ... and with a constant for it
    Ke, konst, pen, words = params(ga, None, 1, 7, [2.5], None, 0)
    assert (Ke, konst, pen) == (1, 1, 2)
    assert as_int64(words[0]) == 7 and as_double(words[1]) == 2.5 and len(words) == 2


def test_tiles(ga):
    assert [ga.ga_tiles(m) for m in (1, 15, 16, 17, 32, 33, 40, 48, 49, 64)] == [1, 1, 1, 2, 2, 3, 3, 3, 4, 4]
