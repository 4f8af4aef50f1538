"""GPU: the fused Gaussian kernel (elfi_amd/csrc/gauss.hip, gauss_kernel) through elfihip_gauss_distance_dev -- the entry
point bench.py times -- at the caller's pitch and alignment, at every length where the row sums change path, at tile
starts that split a Box-Muller pair, with more tiles than workgroups, and at both sides of the longest row the LDS tile
takes; the same long rows through elfihip_row_summary_dev; elfihip_randn_dev into an 8-byte aligned buffer.

Every comparison is bit for bit (np.array_equal): the kernel's contract is NumPy's own summation order on
y = z * sigma + mu (oracle/gauss_oracle.py), and element e of a stream is the same number wherever it is drawn, so the
drawing form (Z == NULL) is compared on what elfihip_randn_dev writes for the same (seed, stream).
"""
import ctypes as C

import numpy as np
import pytest

import distance_oracle as O
import gauss_oracle as GO
from device_layout import LAYOUTS, SENTINEL, guarded_out, place, to_device

pytestmark = pytest.mark.gpu

OBSERVED = (4.0, 0.16)
SEED, STREAM = (0x1234 << 32) | 0x9abcdef1, (7 << 32) | 5      # the high key and counter words are used


def tile_rows(n_obs):
    """gauss_dev_impl's rule: 16 KiB of rows at the LDS pitch n_obs | 1; up to 128 observations eight lanes share a row
    and a tile is a multiple of 16 rows (at least 16), beyond that one lane takes a row and a tile is 1 to 128 rows."""
    rows = (16 * 1024) // ((n_obs | 1) * 8)
    return max(1, min(rows, 128)) if n_obs > 128 else max(16, rows // 16 * 16)


def _sync_in():
    import torch
    torch.cuda.synchronize()     # (torch's stream and the context's own stream are not ordered against each other)


def _params(n, seed):
    rs = np.random.RandomState(seed)
    return rs.uniform(0, 8, n), rs.uniform(0.1, 3, n)


def _oracle(z, mu, sigma):
    y = GO.gauss_from_draws(z, mu, sigma)
    s1, s2 = GO.ss_mean(y), GO.ss_var(y)
    return y, s1, s2, GO.euclidean_to_observed(s1, s2, OBSERVED)


def _place_params(mu, sigma, off):
    """mu and sigma `off` doubles into one buffer, NaN around and between them -> (tensor, address of mu, of sigma)."""
    n = len(mu)
    gap = 2 - n % 2                  # sigma starts at the same parity as mu
    host = np.concatenate([np.full(off, np.nan), mu, np.full(gap, np.nan), sigma, [np.nan]])
    t = to_device(host)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 8 * off, t.data_ptr() + 8 * (off + n + gap)


def _randn(ctx, seed, stream, count):
    """What elfihip_randn_dev writes for (seed, stream): `count` standard normals -> (device tensor, host copy)."""
    import torch
    t = torch.empty(count, dtype=torch.float64, device='cuda')
    _sync_in()
    ctx.call('elfihip_randn_dev', C.c_uint64(seed), C.c_uint64(stream), count, C.c_double(0.0), C.c_double(1.0), t.data_ptr())
    ctx.synchronize()
    return t, t.cpu().numpy()


def _run(ctx, zptr, ldz, n, n_obs, pmu, psigma, with_y=True, out_off=0, seed=0, stream=0):
    """One call of elfihip_gauss_distance_dev into guarded buffers -> (y or None, s1, s2, d); sentinels checked."""
    outs = [guarded_out(n, 1, out_off) for _ in range(3)]
    y = guarded_out(n, n_obs, out_off) if with_y else None
    _sync_in()
    ctx.call('elfihip_gauss_distance_dev', zptr, ldz, C.c_uint64(seed), C.c_uint64(stream), n, n_obs, pmu, psigma,
             C.c_double(OBSERVED[0]), C.c_double(OBSERVED[1]), y.ptr if with_y else None, outs[0].ptr, outs[1].ptr, outs[2].ptr)
    ctx.synchronize()
    got_y = y.check().reshape(n, n_obs) if with_y else None
    return (got_y,) + tuple(o.check() for o in outs)


def _assert_equal(got, ref, what):
    for g, r, name in zip(got, ref, ('y', 'ss_mean', 'ss_var', 'distance')):
        if g is not None:
            assert g.shape == r.shape and np.array_equal(g, r), (name,) + what


@pytest.mark.parametrize('n_obs', [1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 130, 255, 256, 257, 1003])
def test_given_draws_every_layout(hip_ctx, n_obs):
    """Z at the caller's pitch, at an odd pitch and from an 8-byte aligned base (NaN in every gap), mu and sigma and all
    four results from 8-byte aligned addresses, Y asked for and not: the oracle's bits and the packed layout's bits."""
    R = tile_rows(n_obs)
    for n in sorted({1, R - 1, R + 1, 3 * R + R // 2 + 1} - {0}):
        mu, sigma = _params(n, 1000 * n_obs + n)
        z = np.random.RandomState(n_obs + n).standard_normal((n, n_obs))
        ref = _oracle(z, mu, sigma)
        packed = None
        for layout in LAYOUTS:
            pad, off = layout
            buf, zptr = place(z, n_obs + pad, off)
            for out_off in (0, 1):
                par, pmu, psigma = _place_params(mu, sigma, out_off)
                got = _run(hip_ctx, zptr, n_obs + pad, n, n_obs, pmu, psigma, True, out_off)
                _assert_equal(got, ref, (n, n_obs, layout, out_off))
                packed = got if packed is None else packed
                _assert_equal(got, packed, (n, n_obs, layout, out_off, 'the pitch changed the arithmetic'))
            got = _run(hip_ctx, zptr, n_obs + pad, n, n_obs, pmu, psigma, False, 1)
            _assert_equal(got, ref, (n, n_obs, layout, 'Y = NULL'))
            _assert_equal(got, packed, (n, n_obs, layout, 'Y = NULL', 'the pitch changed the arithmetic'))


def _drawn(ctx, n, n_obs, seed, stream):
    """Both runs of the drawing form (Y asked for at an odd offset, Y = NULL) against the oracle on the generator's own
    elements [0, n * n_obs) of the stream."""
    mu, sigma = _params(n, 77 * n_obs + n)
    _, zh = _randn(ctx, seed, stream, n * n_obs)
    ref = _oracle(zh.reshape(n, n_obs), mu, sigma)
    par, pmu, psigma = _place_params(mu, sigma, 1)
    got = _run(ctx, None, 0, n, n_obs, pmu, psigma, True, 1, seed, stream)
    _assert_equal(got, ref, (n, n_obs, 'drawn'))
    got = _run(ctx, None, 0, n, n_obs, pmu, psigma, False, 0, seed, stream)
    _assert_equal(got, ref, (n, n_obs, 'drawn, Y = NULL'))


@pytest.mark.parametrize('n_obs', [129, 257, 2049])
def test_drawn_tiles_that_start_inside_a_pair(hip_ctx, n_obs):
    """Z == NULL, one lane per row: 15, 7 and 1 rows per tile, so every second tile starts at an odd element and the pair
    across its start belongs half to the tile before (the `e >= e0` side of the seam), half to this one."""
    R = tile_rows(n_obs)
    assert R % 2 == 1 and n_obs % 2 == 1
    _drawn(hip_ctx, 5 * R + max(1, R // 2), n_obs, SEED, STREAM)
    _drawn(hip_ctx, 5 * R + max(1, R // 2), n_obs, 42, 9)


@pytest.mark.parametrize('n_obs', [1, 7, 8, 9, 16, 127, 128])
def test_drawn_eight_lane_form_odd_row_counts(hip_ctx, n_obs):
    """Z == NULL, eight lanes per row, an odd number of rows over more than one tile: with an odd n_obs the matrix ends
    inside a pair (the `e < e1` side)."""
    R = tile_rows(n_obs)
    for n in (1, R + 1, 2 * R + 15):
        assert n % 2 == 1
        _drawn(hip_ctx, n, n_obs, SEED, STREAM)


@pytest.mark.parametrize('n_obs', [7, 129, 2049])
def test_more_tiles_than_workgroups(hip_ctx, n_obs):
    """The grid is min(tiles, 8 * cu_count) workgroups: with 8 * cu_count + 3 full tiles and one row more, three
    workgroups run a second trip (four with the ragged last tile) over the LDS tile of their first.  Both forms on the
    same normals, one oracle."""
    cu = hip_ctx.device_info()['cu_count']
    R = tile_rows(n_obs)
    n = R * (8 * cu + 3) + 1
    mu, sigma = _params(n, n_obs)
    zt, zh = _randn(hip_ctx, SEED, STREAM, n * n_obs)
    ref = _oracle(zh.reshape(n, n_obs), mu, sigma)
    par, pmu, psigma = _place_params(mu, sigma, 0)
    got = _run(hip_ctx, None, 0, n, n_obs, pmu, psigma, True, 0, SEED, STREAM)
    _assert_equal(got, ref, (n, n_obs, 'drawn'))
    got = _run(hip_ctx, zt.data_ptr(), n_obs, n, n_obs, pmu, psigma, True, 0)
    _assert_equal(got, ref, (n, n_obs, 'given'))


def _untouched(outs):
    guard = np.float64(SENTINEL).view(np.int64)
    return all(np.all(o.t.cpu().numpy().view(np.int64) == guard) for o in outs)


@pytest.mark.parametrize('n_obs', [8193, 20479])
def test_long_rows_both_forms(hip_ctx, n_obs):
    """8193 observations are the first whose one-row tile is larger than 64 KiB (the kernel opts in to more dynamic LDS),
    20479 the last that fit: (n_obs | 1) * 8 bytes <= 160 KiB.  Both are longer than NumPy's reduction buffer of 8192
    elements, so the oracle's row sums are pairwise inside pieces of 8192 added in order (tests/test_numpy_sum_order.py),
    not one recursion over the row."""
    assert tile_rows(n_obs) == 1 and (n_obs | 1) * 8 > 64 * 1024 and (n_obs | 1) * 8 <= 160 * 1024
    n = 5
    _drawn(hip_ctx, n, n_obs, SEED, STREAM)
    mu, sigma = _params(n, n_obs)
    z = np.random.RandomState(n_obs).standard_normal((n, n_obs))
    ref = _oracle(z, mu, sigma)
    par, pmu, psigma = _place_params(mu, sigma, 1)
    for pad, off in ((0, 0), (1, 0), (3, 1)):
        buf, zptr = place(z, n_obs + pad, off)
        got = _run(hip_ctx, zptr, n_obs + pad, n, n_obs, pmu, psigma, True, 1)
        _assert_equal(got, ref, (n_obs, pad, off))


def test_one_observation_too_many_is_refused(hip_ctx):
    """n_obs = 20480: the pitch 20481 is 8 bytes past 160 KiB.  ELFIHIP_ERR_ARG names the length, nothing is launched:
    no output element is written, in either form."""
    n, n_obs = 3, 20480
    assert (n_obs | 1) * 8 > 160 * 1024 >= ((n_obs - 1) | 1) * 8
    mu, sigma = _params(n, 1)
    par, pmu, psigma = _place_params(mu, sigma, 0)
    buf, zptr = place(np.zeros((n, n_obs)), n_obs, 0)
    for zp in (zptr, None):
        outs = [guarded_out(n) for _ in range(3)] + [guarded_out(n, n_obs)]
        _sync_in()
        with pytest.raises(ValueError, match='20480'):
            hip_ctx.call('elfihip_gauss_distance_dev', zp, n_obs, C.c_uint64(1), C.c_uint64(2), n, n_obs, pmu, psigma,
                         C.c_double(OBSERVED[0]), C.c_double(OBSERVED[1]), outs[3].ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr)
        hip_ctx.synchronize()
        assert _untouched(outs)


SUMMARY_LAYOUTS = [(0, 0), (1, 0), (0, 1), (3, 1)]      # L is odd: pitches L (odd), L + 1 and, from an odd offset, L + 3


@pytest.mark.parametrize('L', [8193, 20479])
def test_row_summary_long_rows(hip_ctx, L):
    """elfihip_row_summary_dev with a one-row tile beyond 64 KiB and at the last length that fits the 160 KiB of LDS."""
    n = 3
    rs = np.random.RandomState(L)
    x = rs.randn(n, L) * rs.uniform(0.1, 50, L) + rs.uniform(-3, 3, L)
    refs = [(0, 0, O.ss_mean(x)), (1, 0, O.ss_var(x)), (2, 1, O.autocov(x, 1)), (2, 7, O.autocov(x, 7))]
    for pad, off in SUMMARY_LAYOUTS:
        buf, ptr = place(x, L + pad, off)
        for kind, lag, ref in refs:
            out = guarded_out(n, 1, off)
            _sync_in()
            hip_ctx.call('elfihip_row_summary_dev', kind, ptr, n, L, L + pad, lag, out.ptr)
            hip_ctx.synchronize()
            assert np.array_equal(out.check(), ref), (L, kind, lag, pad, off)


def test_row_summary_one_value_too_many_is_refused(hip_ctx):
    n, L = 3, 20480
    for pad, off in ((0, 0), (1, 0), (0, 1)):
        buf, ptr = place(np.ones((n, L)), L + pad, off)
        for kind, lag in ((0, 0), (1, 0), (2, 1), (2, 7)):
            out = guarded_out(n)
            _sync_in()
            with pytest.raises(ValueError, match='20480'):
                hip_ctx.call('elfihip_row_summary_dev', kind, ptr, n, L, L + pad, lag, out.ptr)
            hip_ctx.synchronize()
            assert _untouched([out])


@pytest.mark.parametrize('n', [1, 2, 3, 1000, 1001])
def test_randn_into_an_8_byte_aligned_buffer(hip_ctx, n):
    """randn_kernel stores a pair with one 16-byte store only when `out` is 16-byte aligned; from an odd offset every
    element is stored on its own -- the same numbers, nothing outside them."""
    got = []
    for off in (0, 1):
        out = guarded_out(n, 1, off)
        assert out.ptr % 16 == 8 * off
        _sync_in()
        hip_ctx.call('elfihip_randn_dev', C.c_uint64(SEED), C.c_uint64(STREAM), n, C.c_double(-1.5), C.c_double(2.25), out.ptr)
        hip_ctx.synchronize()
        got.append(out.check())
    assert np.array_equal(got[0], got[1])
    _, z = _randn(hip_ctx, SEED, STREAM, n)
    assert np.array_equal(got[0], z * 2.25 + -1.5)      # (multiply and add round separately: gauss.hip contracts nothing)
