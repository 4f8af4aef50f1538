"""Where the host-pointer forms of the example simulators put their arrays in a staging buffer (the layout layer of
elfi_amd/csrc/host_stage.hpp).

That layer is plain C++ (no HIP), so it is compiled here with g++ behind a tiny test-only C wrapper
(tests/cpp/host_stage_capi.cpp) and needs no GPU.  Every expected value below is worked out by hand from the rules:
  absent   a block that is not present takes no room and gets no offset
  aligned  every present block starts at the next multiple of 64 bytes behind the present block before it (the first at 0)
  total    the end of the last present block, not rounded up; 0 when nothing is present
  overflow sizes are size_t; a product, a sum or a rounding that does not fit is refused, not wrapped
"""
import ctypes as C
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ULL = C.c_ulonglong
SIZE_MAX = 2 ** 64 - 1
ABSENT = SIZE_MAX   # what an offset is set to before the call: an absent block's stays


@pytest.fixture(scope='module')
def hs(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('host_stage') / 'libhost_stage_test.so')
    subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-o', out,
                           os.path.join(HERE, 'cpp', 'host_stage_capi.cpp')])
    lib = C.CDLL(out)
    lib.hs_align.restype = ULL
    lib.hs_layout.restype = C.c_int
    lib.hs_layout.argtypes = [C.c_int, C.POINTER(ULL), C.POINTER(ULL), C.POINTER(C.c_int), C.POINTER(ULL), C.POINTER(ULL)]
    return lib


def layout(hs, blocks):
    """blocks: (element size, count, present) -> (offsets with None for an absent block, total), or None on overflow"""
    nb = len(blocks)
    elem, count = (ULL * nb)(*[b[0] for b in blocks]), (ULL * nb)(*[b[1] for b in blocks])
    present, offsets, total = (C.c_int * nb)(*[int(b[2]) for b in blocks]), (ULL * nb)(*[ABSENT] * nb), ULL(ABSENT)
    ok = hs.hs_layout(nb, elem, count, present, offsets, C.byref(total))
    assert ok in (0, 1)
    if not ok:
        return None
    return [None if o == ABSENT else o for o in offsets], total.value


def check_rules(blocks, offsets, total):
    """what holds for any layout: alignment, no overlap, absent blocks nowhere, everything inside the total"""
    spans = []
    for (elem, count, present), off in zip(blocks, offsets):
        assert (off is not None) == bool(present)
        if present:
            assert off % 64 == 0
            spans.append((off, off + elem * count))
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a0 <= a1 <= b0          # in the order given, one behind the other
    assert total == (spans[-1][1] if spans else 0)


def test_header_layout_layer_is_plain_cxx():
    src = open(os.path.join(HERE, '..', 'elfi_amd', 'csrc', 'host_stage.hpp')).read()
    plain = src[:src.index('#if defined(__HIPCC__)')]
    assert 'hip_runtime' not in plain and '#include "' not in plain


def test_alignment_is_64_bytes(hs):
    assert hs.hs_align() == 64


# 3 doubles, 3 int32, 5 int64, 7 bytes: 24, 12, 40 and 7 bytes
FOUR = [(8, 3, True), (4, 3, True), (8, 5, True), (1, 7, True)]


def test_every_block_present(hs):
    offsets, total = layout(hs, FOUR)
    assert offsets == [0, 64, 128, 192] and total == 199
    check_rules(FOUR, offsets, total)


def test_every_block_absent(hs):
    blocks = [(e, c, False) for e, c, _ in FOUR]
    assert layout(hs, blocks) == ([None] * 4, 0)


@pytest.mark.parametrize('gone, want, total', [
    (0, [None, 0, 64, 128], 135),
    (1, [0, None, 64, 128], 135),
    (2, [0, 64, None, 128], 135),
    (3, [0, 64, 128, None], 168),
])
def test_each_single_block_absent(hs, gone, want, total):
    blocks = [(e, c, i != gone) for i, (e, c, _) in enumerate(FOUR)]
    got = layout(hs, blocks)
    assert got == (want, total)
    check_rules(blocks, *got)


def test_odd_counts_of_small_elements_do_not_misalign_what_follows(hs):
    # 3 int32 (12 bytes) before an int64 block: packed, the int64 would start at byte 12
    blocks = [(4, 3, True), (8, 1, True), (1, 65, True), (4, 1, True), (8, 2, True)]
    offsets, total = layout(hs, blocks)
    assert offsets == [0, 64, 128, 256, 320] and total == 336      # 65 bytes take two 64-byte steps
    check_rules(blocks, offsets, total)
    # block order does not matter for alignment: the same blocks reversed
    back = blocks[::-1]
    offsets, total = layout(hs, back)
    assert offsets == [0, 64, 128, 256, 320] and total == 332
    check_rules(back, offsets, total)


def test_block_that_ends_on_a_boundary_is_followed_at_once(hs):
    blocks = [(8, 8, True), (8, 16, True), (4, 1, True)]
    assert layout(hs, blocks) == ([0, 64, 192], 196)


def test_zero_count(hs):
    # a present block of no elements has an offset and no room: the next block starts where it does
    blocks = [(8, 2, True), (4, 0, True), (8, 2, True)]
    offsets, total = layout(hs, blocks)
    assert offsets == [0, 64, 64] and total == 80
    check_rules(blocks, offsets, total)
    assert layout(hs, [(8, 0, True)]) == ([0], 0)


def test_overflow_is_refused(hs):
    assert layout(hs, [(8, SIZE_MAX // 8 + 1, True)]) is None                   # one product
    assert layout(hs, [(8, 1, True), (8, SIZE_MAX // 8, True)]) is None         # the sum
    assert layout(hs, [(1, SIZE_MAX - 10, True), (1, 1, True)]) is None         # the rounding up to 64
    # ... an absent block's size is never formed, and the largest single block fits
    assert layout(hs, [(8, SIZE_MAX // 8 + 1, False), (8, 1, True)]) == ([None, 0], 8)
    assert layout(hs, [(1, SIZE_MAX, True)]) == ([0], SIZE_MAX)
