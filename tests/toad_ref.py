"""NumPy statement of Marchand's toad model as the device runs it (csrc/toad.hip, csrc/stable.hpp; the rule is written
down in include/elfihip.h) -- NumPy only, on top of tests/philox_ref.py.

    draws_from_state(rs, ...)      the reference's own draws, in the order elfi.examples.toad.toad consumes them
    philox_draws(seed, ...)        the device's draws
    stable_step(alpha, scale, TH, W)   SciPy's symmetric alpha-stable transform and a first-order error bound B beside it
    simulate(alpha, gamma, p0, U, dx, R)   the chain of positions
    summaries(X, lag, p, thd)      the len(p) + 1 columns of one lag

Arrays are simulation-major as on the device: draws (batch, n_days - 1, n_toads), X (batch, n_days, n_toads); the
reference's X is (n_days, n_toads, batch).  tests/test_toad.py holds this statement to recorded runs of the reference bit for
bit, the GPU tests hold the device to this statement.
"""
import numpy as np

import philox_ref

EPS = 2.0 ** -52
PI, HALF_PI, TWO_BY_PI = np.pi, np.pi / 2, 2 / np.pi
EXPM20 = np.exp(-20)
TRANSCENDENTAL_ULP = 4.0          # the bound this project holds the device's log and exp to (test_ricker_gpu.py)
NANMEDIAN_SMALL = 600             # np.nanmedian takes its masked-array path below this many values along the axis


def draws_from_state(rs, n_toads=66, n_days=63, batch=1):
    """(U, TH, W, R), each (batch, n_days - 1, n_toads), from a RandomState in the reference's order: per day
    uniform(0, 1, (n_toads, batch)); levy_stable.rvs's uniform.rvs(loc=-pi/2, scale=pi) = uniform pi + (-pi/2) and
    expon.rvs = standard_exponential; choice(i, size=(n_toads, batch))."""
    shape = (n_toads, batch)
    U, TH, W, R = [np.empty((n_days - 1,) + shape) for _ in range(4)]
    for i in range(1, n_days):
        U[i - 1] = rs.uniform(0, 1, shape)
        TH[i - 1] = rs.uniform(size=shape) * PI + (-HALF_PI)
        W[i - 1] = rs.standard_exponential(shape)
        R[i - 1] = rs.choice(i, size=shape)
    return tuple(np.ascontiguousarray(a.transpose(2, 0, 1)) for a in (U, TH, W, R.astype(np.int32)))


def _words(seed, stream, counter):
    u64 = np.uint64
    lo, s32 = u64(0xffffffff), u64(32)
    counter = np.asarray(counter, dtype=u64)
    seed, stream = u64(seed), u64(stream)
    return philox_ref.philox4x32_10_vec((counter & lo, counter >> s32, stream & lo, stream >> s32), (seed & lo, seed >> s32))


def angle_expo(seed, stream, counter):
    """TH and W of Philox counter `counter` of stream (seed, stream): what elfi_amd.levy_stable's element `counter` draws."""
    u64 = np.uint64
    r = _words(seed, stream, counter)
    a, b = (r[0] << u64(21)) | (r[1] >> u64(11)), (r[2] << u64(21)) | (r[3] >> u64(11))
    u1, u2 = a.astype(np.float64) * 2.0 ** -53, (b + u64(1)).astype(np.float64) * 2.0 ** -53
    return u1 * PI + (-HALF_PI), -np.log(u2)


def philox_draws(seed, stream, first_index, n, n_toads=66, n_days=63):
    """The device's (U, TH, W, R), each (n, n_days - 1, n_toads): cell (simulation g = first_index + row, day i, toad j) reads
    the counter e = (g << 32) | (i << 16) | j -- TH, W from stream `stream` as the sampler draws them, U and R from `stream +
    1`: U the 53-bit uniform of words 0, 1, R = (word 2 times i) >> 32."""
    u64 = np.uint64
    g = (np.arange(n, dtype=u64) + u64(first_index))[:, None, None]
    i = np.arange(1, n_days, dtype=u64)[None, :, None]
    j = np.arange(n_toads, dtype=u64)[None, None, :]
    e = (g << u64(32)) | (i << u64(16)) | j
    TH, W = angle_expo(seed, stream, e)
    r = _words(seed, int(stream) + 1, e)
    U = ((r[0] << u64(21)) | (r[1] >> u64(11))).astype(np.float64) * 2.0 ** -53
    R = ((r[2] * i) >> u64(32)).astype(np.int32)
    return U, TH, W, np.broadcast_to(R, U.shape).copy()


def stable_valid(alpha, scale):
    with np.errstate(invalid='ignore'):
        return (alpha > 0) & (alpha <= 2) & (scale >= 0)


def stable_step(alpha, scale, TH, W):
    """(x, B): SciPy 1.15's levy_stable.rvs(alpha, beta=0, scale=scale) on the angle TH and the exponential W (_rvs_Z1's
    beta0func, alpha1func at alpha == 1, then rvs's multiplication by scale), in SciPy's order of operations, and the
    first-order propagation B of an error of TRANSCENDENTAL_ULP ulp per tan / sin / cos / pow call and half an ulp per
    arithmetic operation through that expression (ulp taken as EPS |value|).  Both a NumPy and a device evaluation lie within
    B of the exact value of the expression on the same doubles, hence within 2 B of each other, wherever first order holds;
    where B is large against |x| (the denominator or the numerator cancels) it does not, and callers mask.  Invalid
    parameters give NaN, B = 0."""
    shape = np.broadcast(alpha, scale, TH, W).shape
    # (at least 1-d: an array exponent takes np.power's loop, as SciPy's compressed arrays do, never the scalar fast paths)
    alpha, scale, TH, W = [np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in np.broadcast_arrays(alpha, scale, TH, W)]
    h, t4 = EPS / 2, TRANSCENDENTAL_ULP * EPS
    with np.errstate(all='ignore'):
        ok = stable_valid(alpha, scale)
        one = alpha == 1
        a = np.where(ok & ~one, alpha, 0.5)
        tanTH = np.tan(TH)
        e_tan = t4 * np.abs(tanTH)
        # alpha == 1
        m1 = HALF_PI * tanTH
        z1 = TWO_BY_PI * m1
        e_z1 = e_tan + 2 * h * np.abs(tanTH)
        # alpha != 1
        aTH = a * TH
        e_aTH = h * np.abs(aTH)
        cosTH, sinTH = np.cos(TH), np.sin(TH)
        ta, ca, sa = np.tan(aTH), np.cos(aTH), np.sin(aTH)
        e_ta = t4 * np.abs(ta) + (1 + ta * ta) * e_aTH
        e_ca = t4 * np.abs(ca) + np.abs(sa) * e_aTH
        e_sa = t4 * np.abs(sa) + np.abs(ca) * e_aTH
        q1 = cosTH / ta
        e_q1 = np.abs(q1) * (t4 + e_ta / np.abs(ta) + h)
        den = q1 + sinTH
        e_den = e_q1 + t4 * np.abs(sinTH) + h * np.abs(den)
        v = W / den
        e_v = np.abs(v) * (e_den / np.abs(den) + h)
        pr = sa * tanTH
        e_pr = np.abs(sa) * e_tan + np.abs(tanTH) * e_sa + h * np.abs(pr)
        num = ca + pr
        e_num = e_ca + e_pr + h * np.abs(num)
        r = num / W
        e_r = e_num / W + h * np.abs(r)
        ia = 1.0 / a
        pw = r ** ia
        e_pw = np.abs(pw) * (t4 + ia * e_r / np.abs(r) + np.abs(np.log(r)) * h * ia)
        z = v * pw
        e_z = np.abs(v) * e_pw + np.abs(pw) * e_v + h * np.abs(z)
        Z, e_Z = np.where(one, z1, z), np.where(one, e_z1, e_z)
        x = Z * scale
        B = scale * e_Z + h * np.abs(x)
        x = np.where(ok, x, np.nan)
        B = np.where(ok, B, 0.0)
    return x.reshape(shape), B.reshape(shape)


MASK_RELATIVE = 2.0 ** -20        # elements whose bound exceeds this much of |x| are not compared (first order has ended)
MASK_SHARE = 1e-3                 # ... and they may be at most this share of the elements (the cap the Poisson test uses)


def step_inputs(seed=7):
    """(alpha, scale, TH, W), 30 000 elements, for the sampler's tests on given angles and exponentials: alpha over (0.3, 2],
    the exact values 1 and 2, invalid parameters, and TH pushed towards +-pi/2 (at distances 10^-1 .. 10^-14)."""
    rs = np.random.RandomState(seed)
    n = 30000
    alpha = rs.uniform(0.3, 2.0, n)
    alpha[alpha <= 0.3] = 2.0
    alpha[20000:22000], alpha[22000:24000] = 1.0, 2.0
    scale = rs.uniform(0, 100, n)
    scale[::97] = 0.0
    TH = rs.uniform(size=n) * PI + (-HALF_PI)
    k = np.arange(14000, 21000)                           # alpha over the range, and the head of the alpha == 1 block
    TH[k] = rs.choice([-1.0, 1.0], k.size) * (HALF_PI - 10.0 ** -rs.uniform(1, 14, k.size))
    alpha[14000:14600] = 2.0 - 10.0 ** -rs.uniform(1, 8, 600)      # ... where alpha is close to 2 as well: the sine of alpha TH cancels
    W = rs.standard_exponential(n)
    bad = np.arange(24000, 24600)
    alpha[bad] = np.resize([-1.0, 0.0, 2.5, np.nan, 2.0000000000000004, np.inf, 1.5, 1.5], bad.size)
    scale[bad] = np.resize([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0, np.nan], bad.size)
    return alpha, scale, TH, W


def step_mask(x, B):
    """Elements that are compared: valid parameters and a bound within MASK_RELATIVE of |x|."""
    with np.errstate(invalid='ignore'):
        return np.isfinite(x) & (B <= MASK_RELATIVE * np.abs(x))


def simulate(alpha, gamma, p0, U, dx, R):
    """X (batch, n_days, n_toads): X[0] = 0; a toad with U < p0 returns to X[R], the others move on by dx.  An invalid
    parameter row (alpha outside (0, 2], gamma < 0, p0 outside [0, 1], NaN) is NaN throughout; so is a toad from the day of
    a refuge index outside [0, day)."""
    U, dx, R = np.asarray(U), np.asarray(dx), np.asarray(R)
    n, steps, n_toads = U.shape
    alpha, gamma, p0 = [np.broadcast_to(np.asarray(a, dtype=np.float64).reshape(-1), (n,)) for a in (alpha, gamma, p0)]
    X = np.zeros((n, steps + 1, n_toads))
    rows, toads = np.arange(n)[:, None], np.arange(n_toads)[None, :]
    for i in range(1, steps + 1):
        ret = U[:, i - 1] < p0[:, None]
        r = R[:, i - 1]
        good = (r >= 0) & (r < i)
        back = np.where(good, X[rows, np.where(good, r, 0), toads], np.nan)
        X[:, i] = np.where(ret, back, X[:, i - 1] + dx[:, i - 1])
    with np.errstate(invalid='ignore'):
        X[~(stable_valid(alpha, gamma) & (p0 >= 0) & (p0 <= 1))] = np.nan
    return X


def _lerp_quantiles(v, p):
    """np.quantile(v, p) (method 'linear') of sorted v: the positions elfi_amd.summaries.quantile_positions states, NumPy's _lerp."""
    n = v.shape[0]
    if n == 0:
        return np.full(p.shape, np.nan)
    virt = (n - 1) * p
    prev = np.floor(virt)
    top = virt >= n - 1
    lo = np.where(top, n - 1, prev).astype(np.int64)
    hi = np.where(top, n - 1, prev + 1).astype(np.int64)
    t = virt - np.where(top, -1.0, prev)
    a, b = v[lo], v[np.minimum(hi, n - 1)]
    with np.errstate(invalid='ignore'):
        diff = b - a
        return np.where(t >= 0.5, b - diff * (1 - t), a + diff * t)


def summaries(X, lag, p=None, thd=10.):
    """(batch, len(p) + 1): elfi.examples.toad.compute_summaries of X (batch, n_days, n_toads), as the device computes it --
    the displacements below thd counted, the others (NaN dropped) sorted; np.nanmedian as the mean of the two middle values
    (the single middle value itself from NANMEDIAN_SMALL displacements on: NumPy's two paths differ only when x + x
    overflows), np.nanquantile by positions and _lerp, log(max(diff, exp(-20))), then nan_to_num(nan=inf)."""
    p = np.linspace(0, 1, 11) if p is None else np.asarray(p, dtype=np.float64).reshape(-1)
    X = np.asarray(X)
    n = X.shape[0]
    out = np.empty((n, p.shape[0] + 1))
    with np.errstate(all='ignore'):
        disp = np.abs(X[:, lag:] - X[:, :-lag]).reshape(n, -1)
        m = disp.shape[1]
        for b in range(n):
            d = disp[b]
            ret = d < thd
            v = np.sort(d[~ret & ~np.isnan(d)])
            k = v.shape[0]
            if k == 0:
                med = np.nan
            elif k % 2 and m >= NANMEDIAN_SMALL:
                med = v[k // 2]
            else:
                med = (v[(k - 1) // 2] + v[k // 2]) / 2.0
            q = _lerp_quantiles(v, p)
            out[b, 0], out[b, 1] = ret.sum(), med
            out[b, 2:] = np.log(np.maximum(np.diff(q), EXPM20))
    return np.nan_to_num(out, nan=np.inf)


def all_summaries(X, lags=(1, 2, 4, 8), p=None, thd=10.):
    return np.hstack([summaries(X, lag, p, thd) for lag in lags])


def ulp_distance(a, b):
    """|a - b| in units of the spacing of doubles at max(|a|, |b|)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(all='ignore'):
        return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
