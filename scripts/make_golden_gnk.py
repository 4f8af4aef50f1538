"""Records tests/golden/gnk.npz: ELFI's own g-and-k examples (elfi.examples.gnk / bignk, imported through
oracle/ref_shim.py) run with fixed seeds -- parameters over the models' prior ranges, the MT19937 draws the simulators
consumed, the series, the three reference summaries and euclidean_multiss against the first row.

  gnk     64 simulations x 50 observations          (A, B, g, k ~ U(0, 10))
  bignk   16 simulations x 150 observations x 2     (a, b ~ U(0, 5), g ~ U(-5, 5), k ~ U(-0.5, 5), rho ~ U(-1, 1))

The draws are recorded by replaying the seed through the simulators' own rvs calls (tests/gnk_ref.py); that the replay is
what the simulators consumed is asserted here: the restated series on the replayed draws is the simulators' output bit for
bit.  Beside the reference's series y the file holds it to 40 digits (mpmath, from the same double inputs) as a
double-double pair y_hi + y_lo, and E_ref: the largest error of the reference's own y in units of eps (|A| + |y - A|).

Edge rows (prefix edge_ / biedge_) are the reference's own simulators and summaries on CHOSEN draws, handed to them by a
RandomState whose normal draws are preset: an overflowing exp (g = 400, z <= -2: NaN), B = 0, g = 0, k = -0.5, negative
g, a draw of exactly zero, tied values, rho = +-1.

    python scripts/make_golden_gnk.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

GNK_SEED, BIGNK_SEED, PARAM_SEED, EDGE_SEED = 20271, 20272, 20273, 20274
B1, N1, B2, N2, N3 = 64, 50, 16, 150, 30        # N3: observations of the bivariate edge rows


class Preset(np.random.RandomState):
    """A RandomState whose normal draws are the arrays handed in, in order (SciPy's rvs accept it as a RandomState)."""

    def __init__(self, arrays):
        super().__init__(0)
        self.arrays = list(arrays)

    def standard_normal(self, size=None):
        a = self.arrays.pop(0)
        assert tuple(np.atleast_1d(size)) == a.shape
        return a.copy()

    def multivariate_normal(self, mean, cov, size=None, **kw):
        return self.arrays.pop(0).copy()


def exact(P, z, c=0.8):
    """The series to 40 digits from the same doubles, as a double-double pair."""
    import mpmath as mp
    import gnk_ref as R
    mp.mp.dps = 40
    A, B, g, k = [np.broadcast_to(a, z.shape) for a in R.split_params(P)]
    hi, lo = np.empty(z.shape), np.empty(z.shape)
    cc = mp.mpf(c)
    for i in np.ndindex(z.shape):
        a, b, gg, kk, zz = [mp.mpf(float(v[i])) for v in (A, B, g, k, z)]
        ex = mp.exp(-gg * zz)
        y = a + b * (1 + cc * (1 - ex) / (1 + ex)) * (1 + zz * zz) ** kk * zz
        hi[i] = float(y)
        lo[i] = float(y - mp.mpf(hi[i]))
    return hi, lo


def summaries(gnk, y, prefix, out):
    import gnk_ref as R
    for name, fn, mine in (('order', gnk.ss_order, R.ss_order), ('octile', gnk.ss_octile, R.ss_octile),
                           ('robust', gnk.ss_robust, R.ss_robust)):
        with np.errstate(all='ignore'):
            s = fn(y)
            assert np.array_equal(s, mine(y), equal_nan=True), name
            out[prefix + '_d_' + name] = gnk.euclidean_multiss(s, observed=(s[:1],))
            if name == 'order':
                # ss_order sorts the values of ONE observation: its output is y with some pairs swapped (none at dim = 1),
                # and is recorded as that mask (gnk_ref.order_from_swaps) -- a second copy of y would double the file
                swaps = ~((s[:, :, 0] == y[:, :, 0]) | (np.isnan(s[:, :, 0]) & np.isnan(y[:, :, 0])))
                assert np.array_equal(R.order_from_swaps(y, swaps), s, equal_nan=True)
                out[prefix + '_order_swaps'] = swaps
            else:
                out[prefix + '_' + name] = s


def main():
    import ref_shim
    ref_shim.install()
    from elfi.examples import bignk, gnk
    import gnk_ref as R
    rs = np.random.RandomState(PARAM_SEED)
    out = {}

    P = rs.uniform(0, 10, (B1, 4))
    y = gnk.GNK(*P.T, n_obs=N1, batch_size=B1, random_state=np.random.RandomState(GNK_SEED))
    z = R.gnk_draws_from_state(np.random.RandomState(GNK_SEED), B1, N1)
    assert y.shape == (B1, N1, 1) and np.array_equal(R.series(P, z), y), 'the replayed draws are not what GNK consumed'
    hi, lo = exact(P, z[:, :, None])
    out.update(gnk_P=P, gnk_z=z, gnk_y=y, gnk_y_hi=hi, gnk_y_lo=lo)
    summaries(gnk, y, 'gnk', out)

    eps = np.finfo(float).eps
    P2 = np.column_stack([rs.uniform(0, 5, (B2, 4)), rs.uniform(-5, 5, (B2, 2)), rs.uniform(-.5, 5, (B2, 2)),
                          rs.uniform(-1 + eps, 1 - eps, B2)])
    y2 = bignk.BiGNK(*P2.T, n_obs=N2, batch_size=B2, random_state=np.random.RandomState(BIGNK_SEED))
    z2 = R.bignk_draws_from_state(np.random.RandomState(BIGNK_SEED), P2[:, 8], N2)
    assert y2.shape == (B2, N2, 2) and np.array_equal(R.series(P2, z2), y2), 'the replayed draws are not what BiGNK consumed'
    hi2, lo2 = exact(P2, z2)
    out.update(bignk_P=P2, bignk_z=z2, bignk_y=y2, bignk_y_hi=hi2, bignk_y_lo=lo2)
    summaries(gnk, y2, 'bignk', out)
    out['E_ref'] = R.e_ref(out)

    # ---- edge rows: the reference's own functions on chosen draws ----
    es = np.random.RandomState(EDGE_SEED)
    names = ['plain', 'overflow', 'plain2', 'B0', 'g0', 'kneg', 'gneg', 'zero', 'ties', 'g400_finite']
    Pe = np.tile([3.0, 1.0, 2.0, 0.5], (len(names), 1))
    ze = es.standard_normal((len(names), N1))
    Pe[1, 2] = 400.0
    ze[1] = np.maximum(ze[1], -1.7)          # exp(-400 z) overflows below z = -1.7745
    ze[1, 3], ze[1, 10], ze[1, 49] = -2.0, -2.5, -3.25
    Pe[3, 1] = 0.0
    Pe[4, 2] = 0.0
    Pe[5, 3] = -0.5
    Pe[6, 2] = -3.0
    ze[7, 5], ze[7, 6] = 0.0, -0.0
    ze[8, :10], ze[8, 20:24] = ze[8, 0], ze[8, 20]
    Pe[9, 2] = 400.0
    ze[9] = np.maximum(ze[9], -1.7)
    with np.errstate(all='ignore'):
        ye = gnk.GNK(*Pe.T, n_obs=N1, batch_size=len(names), random_state=Preset([ze]))
    assert np.array_equal(R.series(Pe, ze), ye, equal_nan=True)
    assert np.array_equal(np.argwhere(np.isnan(ye[:, :, 0])), [[1, 3], [1, 10], [1, 49]])
    out.update(edge_names=np.array(names), edge_P=Pe, edge_z=ze, edge_y=ye)
    summaries(gnk, ye, 'edge', out)

    binames = ['plain', 'rho_plus', 'rho_minus', 'overflow_d0', 'ties']
    Pb = np.tile([3, 4, 1, 0.5, 1, 2, .5, .4, 0.6], (len(binames), 1))
    e = es.standard_normal((len(binames), N3, 2))
    Pb[1, 8], Pb[2, 8] = 1.0, -1.0
    zb = R.correlate(e, Pb[:, 8])
    assert np.array_equal(zb[1, :, 1], zb[1, :, 0]) and np.array_equal(zb[2, :, 1], -zb[2, :, 0])
    Pb[3, 4] = 400.0
    zb[3, 7, 0], zb[3, 29, 0] = -2.0, -4.0
    zb[4, :12, 1] = zb[4, 0, 1]
    with np.errstate(all='ignore'):
        yb = bignk.BiGNK(*Pb.T, n_obs=N3, batch_size=len(binames), random_state=Preset(list(zb)))
    assert np.array_equal(R.series(Pb, zb), yb, equal_nan=True)
    assert np.array_equal(np.argwhere(np.isnan(yb)), [[3, 7, 0], [3, 29, 0]])
    out.update(biedge_names=np.array(binames), biedge_P=Pb, biedge_z=zb, biedge_y=yb)
    summaries(gnk, yb, 'biedge', out)

    path = os.path.join(ROOT, 'tests', 'golden', 'gnk.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, 'bytes; E_ref =', out['E_ref'])
    assert size < 300 * 1024


if __name__ == '__main__':
    main()
