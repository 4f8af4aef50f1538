"""Writes tests/golden/special_fn.npz: Owen's T, the normal cdf and the MaxVar kernel W with its partial derivatives at
50 digits (mpmath), on the (z, b) grid the device tests of the MaxVar family sweep (tests/test_maxvar_surfaces_gpu.py).

    T(h, a)  = (1 / 2 pi) int_0^a exp(-h^2 (1 + x^2) / 2) / (1 + x^2) dx                       [Owen 1956]
    Phi(z)   = erfc(-z / sqrt 2) / 2
    W(z, b)  = Phi(z) Phi(-z) - 2 T(z, b) = (1 / pi) int_b^1 exp(-z^2 (1 + x^2) / 2) / (1 + x^2) dx
               (T(z, 1) = Phi(z) Phi(-z) / 2; the second form has no cancellation and is the one integrated)
    dW / dz  = 2 phi(z) (Phi(b z) - Phi(z))
    dW / db  = -exp(-z^2 (1 + b^2) / 2) / (pi (1 + b^2))

Both integrals are taken by mpmath's tanh-sinh rule over sub-intervals that double in width away from the end where the
integrand is largest, with mpmath's own error estimate; the script FAILS if an estimate exceeds 1e-25 of the value, or if
T(h, 1) differs from Phi(h) Phi(-h) / 2, or the two forms of W differ, by more than that.  The arguments are the binary64
numbers stored in the file, so the values are those of the functions AT the stored arguments, rounded once to binary64.

Only z >= 0 is integrated: T and W are even in z, dW/dz is odd, dW/db is even.

    python oracle/make_golden_special.py            # writes the file
    python oracle/make_golden_special.py --check    # recomputes and compares with the file, value by value
"""
import os
import sys

import mpmath as mp
import numpy as np

mp.mp.dps = 50
REL_TOL = mp.mpf(10) ** -25

ZABS = [0.0, 1e-3, 0.5, 1.0, 2.0, 3.0, 4.5, 6.0, 9.0, 12.0, 20.0, 28.0, 37.0, 38.0]
A = [0.0, 1e-8, 1e-3, 1e-2, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 1.0 - 1e-4, 1.0 - 1e-6, 1.0 - 1e-9, 1.0]

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'special_fn.npz')


def Phi(z):
    return mp.erfc(-z / mp.sqrt(2)) / 2


def phi(z):
    return mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi)


def integral(h, lo, hi):
    """int_lo^hi exp(-h^2 (1 + x^2) / 2) / (1 + x^2) dx with a checked error estimate."""
    if hi == lo:
        return mp.mpf(0)
    # (the factor exp(-h^2 (1 + lo^2) / 2) is taken out, so that the estimate is relative to a value of order one)
    f = lambda x: mp.exp(-h * h * (x * x - lo * lo) / 2) / (1 + x * x)
    # the integrand falls from `lo` on like exp(-h^2 (x^2 - lo^2) / 2): first sub-interval of that length, then doubling
    step = hi - lo
    if h != 0:
        step = min(step, 1 / abs(h), 1 / (h * h * lo) if lo > 0 else step)
    pts, x = [lo], lo
    while x + step < hi:
        x = x + step
        pts.append(x)
        step = 2 * step
    pts.append(hi)
    val, err = mp.quad(f, pts, error=True, maxdegree=10)
    if not err <= REL_TOL * abs(val):
        raise SystemExit('integral(h=%s, %s, %s): error estimate %s exceeds 1e-25 of %s'
                         % (mp.nstr(h, 5), mp.nstr(lo, 12), mp.nstr(hi, 12), mp.nstr(err, 3), mp.nstr(val, 5)))
    return val * mp.exp(-h * h * (1 + lo * lo) / 2)


def compute():
    nz, na = len(ZABS), len(A)
    T, W, dWz, dWb = (np.empty((nz, na)) for _ in range(4))
    worst_self = mp.mpf(0)
    for i, zf in enumerate(ZABS):
        z = mp.mpf(zf)
        Pz, Pm = Phi(z), Phi(-z)
        t1 = integral(z, mp.mpf(0), mp.mpf(1)) / (2 * mp.pi)
        worst_self = max(worst_self, abs(t1 - Pz * Pm / 2) / (Pz * Pm / 2))
        for j, af in enumerate(A):
            a = mp.mpf(af)
            t = integral(z, mp.mpf(0), a) / (2 * mp.pi)
            w = integral(z, a, mp.mpf(1)) / mp.pi
            # the two forms of W: the difference carries the cancellation, so it is compared on the scale of its terms
            worst_self = max(worst_self, abs((Pz * Pm - 2 * t) - w) / (Pz * Pm))
            T[i, j], W[i, j] = float(t), float(w)
            dWz[i, j] = float(2 * phi(z) * (Phi(a * z) - Pz))
            dWb[i, j] = float(-mp.exp(-z * z * (1 + a * a) / 2) / (mp.pi * (1 + a * a)))
    if not worst_self <= REL_TOL:
        raise SystemExit('self-check failed: %s' % mp.nstr(worst_self, 3))
    # mirror to negative z
    zs = np.array([-v for v in ZABS[:0:-1]] + ZABS)
    m = lambda X, sign: np.concatenate([sign * X[:0:-1], X], axis=0)
    P = np.array([float(Phi(mp.mpf(float(v)))) for v in zs])
    return dict(z=zs, a=np.array(A), T=m(T, 1.0), Phi=P, W=m(W, 1.0), dW_dz=m(dWz, -1.0), dW_db=m(dWb, 1.0),
                digits=np.array(mp.mp.dps), rel_err_bound=np.array(float(REL_TOL)))


def main(argv):
    got = compute()
    if '--check' in argv:
        have = np.load(OUT)
        for k, v in got.items():
            if not np.array_equal(have[k], v):
                raise SystemExit('%s differs from %s' % (k, OUT))
        print('identical:', OUT)
        return
    np.savez(OUT, **got)
    print('wrote %s (%d bytes)' % (OUT, os.path.getsize(OUT)))


if __name__ == '__main__':
    main(sys.argv[1:])
