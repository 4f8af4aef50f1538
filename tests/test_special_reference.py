"""The references of the MaxVar-family device tests, held to 50-digit values (tests/golden/special_fn.npz, written by
oracle/make_golden_special.py with mpmath; error estimate of every integral <= 1e-25 relative).

tests/test_maxvar_surfaces_gpu.py compares the device's Owen's T and W = Phi(z) Phi(-z) - 2 T(z, b) with
scipy.special.owens_t / ndtr at absolute tolerances of 1e-12 (surface) and 1e-13 (ExpIntVar loss).  What SciPy itself is
worth cannot be derived beforehand, so it is MEASURED against the fixture and the assertion is 4 x the measurement (another
SciPy build may round differently); see the constants below.  The same file transcribes the quadrature of
elfi_amd/csrc/special.hpp into NumPy and measures the accuracy of that DESIGN (panel rule, 10-point nodes), which is what
the header's accuracy statement now quotes.
"""
import math
import os

import numpy as np
from scipy.special import ndtr, owens_t

from conftest import GOLDEN

# |h| ranges of the relative figures (T falls like exp(-h^2 / 2): 5e-298 at |h| = 37, subnormal at 38)
H_RANGES = ((0.0, 1.0), (1.0, 6.0), (6.0, 12.0), (12.0, 20.0), (20.0, 28.0), (28.0, 37.0))

# measured on SciPy 1.15.3 / NumPy 2.2.6 against the fixture (worst over the grid); asserted: 4 x these
SCIPY_T_ABS = 4.2e-17        # |owens_t - T|
SCIPY_T_REL = 1.7e-9        # the same relative to T, |h| <= 37
SCIPY_PHI_REL = 1.2e-13      # |ndtr - Phi| / Phi, |z| <= 37
SCIPY_W_ABS = 7.5e-17        # |ndtr(z) ndtr(-z) - 2 owens_t(z, b) - W|: the form the device tests use
# the device tolerances that rest on SciPy (absolute, for p = 1 and sum |w| = 1)
DEVICE_SURFACE_TOL, DEVICE_LOSS_TOL = 1e-12, 1e-13

# measured for the NumPy transcription of special.hpp's quadrature (host libm exp); asserted: 4 x these
QUAD_T_ABS = 1.1e-14
QUAD_T_REL = (1.6e-13, 1.6e-13, 4.3e-15, 1.1e-14, 1.3e-14, 2.3e-14)   # worst relative error per range of H_RANGES
QUAD_W_ABS = 2.1e-14


def _fixture():
    g = np.load(os.path.join(GOLDEN, 'special_fn.npz'))
    Z, A = np.meshgrid(g['z'], g['a'], indexing='ij')
    return g, Z, A


_GX = (0.14887433898163121088, 0.43339539412924719080, 0.67940956829902440623, 0.86506336668898451073,
       0.97390652851717172008)
_GW = (0.29552422471475287017, 0.26926671930999635509, 0.21908636251598204400, 0.14945134915058059315,
       0.06667134430868813759)


def _owens_t_one(h, a):
    """elfi_amd/csrc/special.hpp owens_t, statement by statement, in binary64."""
    if not a > 0.0:
        return 0.0
    ah = abs(h) * a
    panels = min(96, 1 + int(0.75 * ah))
    w, hh = a / panels, -0.5 * h * h
    total = 0.0
    for p in range(panels):
        mid, half = (p + 0.5) * w, 0.5 * w
        s = 0.0
        for gx, gw in zip(_GX, _GW):
            x1, x2 = mid - half * gx, mid + half * gx
            q1, q2 = 1.0 + x1 * x1, 1.0 + x2 * x2
            s += gw * (math.exp(hh * q1) / q1 + math.exp(hh * q2) / q2)
        total += s * half
    return total * 0.15915494309189533577


def owens_t_device_form(h, a):
    h, a = np.broadcast_arrays(np.asarray(h, float), np.asarray(a, float))
    return np.array([_owens_t_one(float(x), float(y)) for x, y in zip(h.ravel(), a.ravel())]).reshape(h.shape)


def _rel_by_range(t, g, Z):
    ref = g['T']
    rel = np.abs(t - ref) / np.where(ref > 0, ref, 1.0)
    out = []
    for lo, hi in H_RANGES:
        m = (np.abs(Z) >= lo) & (np.abs(Z) <= hi) & (ref > 0)
        out.append(float(np.max(rel[m])))
    return out


def test_the_fixture_is_what_the_script_describes():
    g, Z, A = _fixture()
    assert int(g['digits']) >= 40 and float(g['rel_err_bound']) <= 1e-25
    z, a = g['z'], g['a']
    # the grid of the device sweep: z = 0 exactly, |z| in {1e-3, 1, 3, 6, 9, 20, 37}, out to 38; a = 0, 1e-8, 1 and b from
    # 1e-3 to 1 - 1e-9
    for v in (0.0, 1e-3, 1.0, 3.0, 6.0, 9.0, 20.0, 37.0, 38.0):
        assert v in z and -v in z
    for v in (0.0, 1e-8, 1e-3, 1.0 - 1e-9, 1.0):
        assert v in a
    # identities that hold to the last bit of a correctly rounded table: T(h, 0) = 0, W(z, 1) = 0, T even in h
    assert np.all(g['T'][:, 0] == 0.0) and np.all(g['W'][:, -1] == 0.0)
    assert np.array_equal(g['T'], g['T'][::-1]) and np.array_equal(g['dW_dz'], -g['dW_dz'][::-1])
    assert np.all(g['W'] >= 0.0) and np.all(g['dW_db'] <= 0.0)


def test_scipy_owens_t_and_ndtr_against_the_fixture():
    """Measured here (SciPy 1.15.3): owens_t absolute 4.2e-17, relative 1.7e-9 over |h| <= 37; ndtr relative
    1.2e-13; the W form absolute 7.5e-17.  Asserted at 4 x each.  The device tolerances (1e-12 on the
    surface, 1e-13 on the loss) stay more than 4 x above the absolute figures, so they are not widened."""
    g, Z, A = _fixture()
    t = owens_t(Z, A)
    err = np.abs(t - g['T'])
    print('scipy owens_t: abs %.3g, rel by |h| range %s' % (err.max(), _rel_by_range(t, g, Z)))
    assert err.max() <= 4 * SCIPY_T_ABS
    assert max(_rel_by_range(t, g, Z)) <= 4 * SCIPY_T_REL
    m = np.abs(g['z']) <= 37
    prel = np.max(np.abs(ndtr(g['z']) - g['Phi'])[m] / g['Phi'][m])
    print('scipy ndtr: rel %.3g' % prel)
    assert prel <= 4 * SCIPY_PHI_REL
    w = ndtr(Z) * ndtr(-Z) - 2.0 * t
    werr = np.max(np.abs(w - g['W']))
    print('W form: abs %.3g' % werr)
    assert werr <= 4 * SCIPY_W_ABS
    assert DEVICE_SURFACE_TOL >= 4 * 4 * SCIPY_W_ABS and DEVICE_LOSS_TOL >= 4 * 4 * 2 * SCIPY_T_ABS


def test_the_chain_rule_of_the_surface_against_the_fixture():
    """dW/dz and dW/db as the kernel's header writes them (dT/dh = -phi(h) (Phi(a h) - 1/2), dT/da = exp(-h^2 (1 + a^2) / 2)
    / (2 pi (1 + a^2))) in SciPy arithmetic: the reference of the device gradient test.  The terms of dW/dz cancel, so the
    error is taken on the scale of their absolute sum (what the device test uses as its allowance, at 1e-11)."""
    g, Z, A = _fixture()
    pz = np.exp(-0.5 * Z * Z) / np.sqrt(2 * np.pi)
    Pz = ndtr(Z)
    dT_dh = -pz * (ndtr(Z * A) - 0.5)
    dT_da = np.exp(-0.5 * Z * Z * (1 + A * A)) / (2 * np.pi * (1 + A * A))
    dW_dz = (1 - 2 * Pz) * pz - 2 * dT_dh
    scale = np.abs(1 - 2 * Pz) * pz + 2 * np.abs(dT_dh)
    m = np.abs(Z) <= 37                  # (phi(38) = 1e-314 is subnormal: no relative precision left to compare)
    e1 = np.max((np.abs(dW_dz - g['dW_dz']) / np.where(scale > 0, scale, 1.0))[m])
    ref_b = g['dW_db']
    e2 = np.max((np.abs(-2 * dT_da - ref_b) / np.where(ref_b < 0, -ref_b, 1.0))[m])
    assert np.max(np.abs(dW_dz - g['dW_dz'])[~m]) <= 1e-300 and np.max(np.abs(-2 * dT_da - ref_b)[~m]) <= 1e-300
    print('dW/dz %.3g of the terms, dW/db rel %.3g' % (e1, e2))
    # binary64 arithmetic of a handful of operations; exp(-x) carries x ulp of relative error, x <= 1444: 3.2e-13
    assert e1 <= 1e-12 and e2 <= 1e-12


def test_quadrature_of_special_hpp_against_the_fixture():
    """The accuracy of the device's quadrature DESIGN: Gauss-Legendre panels of ten points, 1 + floor(0.75 |h| a) of them (at
    most 96).  Measured (host exp): absolute 1.1e-14; relative per |h| range see QUAD_T_REL; W form absolute
    2.1e-14.  These are the figures elfi_amd/csrc/special.hpp and DESIGN.md quote."""
    g, Z, A = _fixture()
    t = owens_t_device_form(Z, A)
    err = np.abs(t - g['T'])
    rel = _rel_by_range(t, g, Z)
    k = int(np.argmax(np.where((np.abs(Z) <= 37) & (g['T'] > 0), err / np.where(g['T'] > 0, g['T'], 1.0), 0.0)))
    print('quadrature: abs %.3g; rel by |h| range %s; worst at h = %g, a = %r' % (err.max(), rel, Z.flat[k], A.flat[k]))
    assert err.max() <= 4 * QUAD_T_ABS
    for r, m in zip(rel, QUAD_T_REL):
        assert r <= 4 * m
    w = ndtr(Z) * ndtr(-Z) - 2.0 * t
    assert np.max(np.abs(w - g['W'])) <= 4 * QUAD_W_ABS
    assert DEVICE_SURFACE_TOL >= 4 * QUAD_W_ABS and DEVICE_LOSS_TOL >= 4 * 2 * QUAD_T_ABS
    # a = 0 and a = 1e-8: one panel, T = a exp(-h^2 / 2) / 2 pi to first order
    assert np.all(t[:, 0] == 0.0)
