"""Records tests/golden/wsemibsl.npz: the whitened semiparametric synthetic likelihood (wsemiBSL) of the cases of
tests/wsemibsl_ref.py (run where the reference is installed; oracle/ref_shim.py makes it importable; np.NINF is aliased in
this process as in scripts/make_golden_semibsl.py).

Per case (wsemibsl_ref.variants() x CONFIGS) it stores
  truth    the likelihood of the same float inputs (X, y, W) in 60-digit arithmetic, as a double-double (hi, lo): exact
           ranks, Phi^-1 at the exact rational, T = Q W^T exact to 60 digits, the ranks of T's columns from those values,
  e_np     |wsemibsl_ref.wsemi_loglik_ref - truth|,
  e_ref    |pdf_methods.semi_param_kernel_estimate(whitening=W) - truth|, NaN where that function does not run (one
           summary: it squeezes ssy to 0-d),
  gap      the smallest gap between neighbouring values within a column of the 60-digit T, relative to the column's range,
           rows that come from equal rows of Q counting as one value,
  rho, scale and their e_np: the 60-digit rank correlation (unshrunk) and d rounded to double, and the largest error of
           the NumPy statement's.
A fixture with a gap below wsemibsl_ref.MIN_GAP is not written: rounding at the 1e-16 level could change a rank, and the
truth would not be the one answer.  Inputs are not stored: the tests regenerate them from the recipe.

    python scripts/make_golden_wsemibsl.py
"""
import math
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'oracle'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'scripts')):
    sys.path.insert(0, p)
import ref_shim  # noqa: E402
import semibsl_ref as S  # noqa: E402
import wsemibsl_ref as R  # noqa: E402
from make_golden_semibsl import mp_ppf, split  # noqa: E402

mp.mp.dps = 60
mpf = mp.mpf


def column_gap(T, Q):
    """The smallest gap between neighbouring values within a column of T, relative to the column's range; rows of T that
    come from equal rows of Q are one value.  T may hold numbers of any type that sorts and subtracts."""
    gap = math.inf
    for j in range(len(T[0])):
        order = sorted(range(len(T)), key=lambda i: T[i][j])
        width = T[order[-1]][j] - T[order[0]][j]
        for a, b in zip(order[:-1], order[1:]):
            if not np.array_equal(Q[a], Q[b]):
                gap = min(gap, float((T[b][j] - T[a][j]) / width))
    return gap


def ranks_of(values):
    """1-based ranks with ties at the average rank, of a list of mpf."""
    return [sum(1 for t in values if t < v) + (sum(1 for t in values if t == v) + 1) / 2.0 for v in values]


def scores_of(ranks, n, table):
    out = []
    for r in ranks:
        r = float(r)
        if r not in table:
            table[r] = mp_ppf(mpf(r) / (n + 1))
        out.append(table[r])
    return out


def truth_parts(X, y, W):
    """(sum of logpdf, eta_w, rho unshrunk, d, gap) in mpmath."""
    n, m = X.shape
    Wm = [[mpf(float(v)) for v in row] for row in W]
    lp, eta, Q, table = mpf(0), [], [], {}
    for j in range(m):
        col = [mpf(float(v)) for v in X[:, j]]
        mu = mp.fsum(col) / n
        var = mp.fsum((v - mu) ** 2 for v in col) / (n - 1)
        h = (mpf(3) * n / 4) ** (mpf(-1) / 5) * mp.sqrt(var)
        zs = [(mpf(float(y[j])) - v) / h for v in col]
        lp += mp.log(mp.fsum(mp.exp(-z * z / 2) for z in zs) / n / h / mp.sqrt(2 * mp.pi))
        eta.append(mp_ppf(mp.fsum(mp.ncdf(z) for z in zs) / n))
        Q.append(scores_of(S.ranks(X[:, j]), n, table))
    rows = [[Q[j][i] for j in range(m)] for i in range(n)]
    T = [[mp.fdot(rows[i], Wm[a]) for a in range(m)] for i in range(n)]
    gap = column_gap(T, np.column_stack([S.ranks(X[:, j]) for j in range(m)]))
    Q2 = [scores_of(ranks_of([T[i][a] for i in range(n)]), n, table) for a in range(m)]
    den = mp.fsum(mp_ppf(mpf(i) / (n + 1)) ** 2 for i in range(1, n + 1))
    rho = [[mpf(1) if a == b else None for b in range(m)] for a in range(m)]
    mean = [mp.fsum(Q[a]) / n for a in range(m)]
    Qc = [[v - mean[a] for v in Q[a]] for a in range(m)]
    C = [[None] * m for _ in range(m)]
    for a in range(m):
        for b in range(a + 1):
            C[a][b] = C[b][a] = mp.fdot(Qc[a], Qc[b]) / (n - 1)
            if b < a:
                rho[a][b] = rho[b][a] = mp.fdot(Q2[a], Q2[b]) / den
    d = [mp.sqrt(mp.fdot(Wm[a], [mp.fdot(C[b], Wm[a]) for b in range(m)])) for a in range(m)]
    eta_w = [mp.fdot(Wm[a], eta) for a in range(m)]
    return lp, eta_w, rho, d, gap


def truth_loglik(parts, penalty=None):
    lp, ew, rho, d, _ = parts
    m = len(ew)
    g = mpf(1) if penalty is None else 1 - mpf(float(penalty))
    M = [[d[a] * d[b] * (mpf(1) if a == b else g * rho[a][b]) for b in range(m)] for a in range(m)]
    L = [[mpf(0)] * m for _ in range(m)]
    for j in range(m):
        piv = M[j][j] - mp.fsum(L[j][k] * L[j][k] for k in range(j))
        assert piv > 0
        L[j][j] = mp.sqrt(piv)
        for i in range(j + 1, m):
            L[i][j] = (M[i][j] - mp.fdot(L[i][:j], L[j][:j])) / L[j][j]
    z = []
    for i in range(m):
        z.append((ew[i] - mp.fdot(L[i][:i], z)) / L[i][i])
    logdet = 2 * mp.fsum(mp.log(L[j][j]) for j in range(m))
    return -(logdet + mp.fsum(v * v for v in z) - mp.fsum(v * v for v in ew)) / 2 + lp


def main():
    ref_shim.install()
    np.NINF = -np.inf           # pdf_methods.py:229 still uses the name
    from elfi.methods.bsl import pdf_methods as P
    variants = R.variants()
    shape = (len(variants), len(R.CONFIGS))
    hi, lo, e_np, e_ref = (np.full(shape, np.nan) for _ in range(4))
    gap, e_rho, e_scale = (np.full(len(variants), np.nan) for _ in range(3))
    rho_t, scale_t = np.full((len(variants), 64, 64), np.nan), np.full((len(variants), 64), np.nan)
    for vi, (ci, tied) in enumerate(variants):
        X, y, W = R.make_case(ci, tied)
        n, m = X.shape
        parts = truth_parts(X, y, W)
        gap[vi] = parts[4]
        rho_t[vi, :m, :m] = [[float(v) for v in row] for row in parts[2]]
        scale_t[vi, :m] = [float(v) for v in parts[3]]
        _, _, rho_np, d_np, _, _ = R.wparts(X, y, W)
        e_rho[vi] = max(float(abs(mpf(float(rho_np[a, b])) - parts[2][a][b])) for a in range(m) for b in range(m))
        e_scale[vi] = max(float(abs(mpf(float(d_np[a])) - parts[3][a])) for a in range(m))
        for ki, pen in enumerate(R.CONFIGS):
            kw = {} if pen is None else dict(shrinkage='warton', penalty=pen)
            t = truth_loglik(parts, pen)
            hi[vi, ki], lo[vi, ki] = split(t)
            e_np[vi, ki] = float(abs(mpf(float(R.wsemi_loglik_ref(X, y, W, **kw))) - t))
            if m > 1:
                r = float(np.ravel(P.semi_param_kernel_estimate(X, y, whitening=W, **kw))[0])
                e_ref[vi, ki] = float(abs(mpf(r) - t))
            print('n=%d m=%d %s penalty %-4s truth % .17g  e_np %.2e  e_ref %.2e  gap %.2e  e_rho %.2e  e_scale %.2e'
                  % (n, m, 'tied ' if tied else 'plain', pen, hi[vi, ki], e_np[vi, ki], e_ref[vi, ki], gap[vi], e_rho[vi],
                     e_scale[vi]), flush=True)
    if not np.all(gap >= R.MIN_GAP):
        sys.exit('a case has a column gap below %g: change its seed (wsemibsl_ref.SEEDS); nothing written' % R.MIN_GAP)
    path = os.path.join(ROOT, 'tests', 'golden', 'wsemibsl.npz')
    np.savez_compressed(path, variants=np.array([(ci, int(t)) for ci, t in variants]), configs=np.array([np.nan, 0.4]),
                        truth_hi=hi, truth_lo=lo, e_np=e_np, e_ref=e_ref, gap=gap, rho=rho_t, scale=scale_t, e_rho=e_rho,
                        e_scale=e_scale)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
