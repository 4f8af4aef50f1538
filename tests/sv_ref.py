"""NumPy statement of the alpha-stable stochastic-volatility model as the device runs it (csrc/sv.hip, csrc/stable.hpp; the
rule is written down in include/elfihip.h) -- NumPy only, on top of tests/philox_ref.py and tests/toad_ref.py.

    draws_from_state(rs, n_obs, batch)   the reference's own draws, in the order its simulator consumes them
    philox_draws(seed, ...)              the device's draws
    stable_general_step(alpha, beta, loc, scale, TH, W, parameterization)
                                         SciPy's levy_stable.rvs on an angle and an exponential, and a first-order bound B
    log_vol(mu, phi, sigma, Z, x_0)      the AR(1) chain of log-volatilities
    returns(x, v), summaries(y)          y = exp(x / 2) v and the quantile-based kurtosis and skewness

Arrays are simulation-major as on the device: draws, x, v, y are (batch, n_obs); the reference's are (n_obs, batch) inside
its simulator.  tests/test_sv.py holds this statement to recorded runs of the reference bit for bit, the GPU tests hold the
device to this statement.
"""
import numpy as np

import toad_ref
from toad_ref import EPS, HALF_PI, MASK_RELATIVE, MASK_SHARE, PI, TRANSCENDENTAL_ULP, TWO_BY_PI, ulp_distance  # noqa: F401

Q_KURT = (0.05, 0.25, 0.75, 0.95)
Q_SKEW = (0.05, 0.5, 0.95)
PHI_SQUARE_CAP = 0.99999


def draws_from_state(rs, n_obs=50, batch=1):
    """(Z, TH, W), each (batch, n_obs), from a RandomState in the reference's order: log_vol's n_obs calls of
    ss.norm.rvs(size=batch) = standard_normal(batch) (times scale, plus loc), then levy_stable.rvs(size=(n_obs, batch)):
    uniform.rvs(loc=-pi/2, scale=pi) = uniform pi + (-pi/2), and expon.rvs = standard_exponential."""
    Z = np.empty((n_obs, batch))
    for t in range(n_obs):
        Z[t] = rs.standard_normal(batch)
    TH = rs.uniform(size=(n_obs, batch)) * PI + (-HALF_PI)
    W = rs.standard_exponential((n_obs, batch))
    return tuple(np.ascontiguousarray(a.T) for a in (Z, TH, W))


def _cospi(v):
    """cos(pi v) for v in [0, 2]: the argument is reduced exactly to |r| <= 1/4 before pi enters, and pi enters with its
    second word in extended precision (where the platform has one), so the result is the rounded cosine but for the last bit."""
    k = np.rint(2.0 * v)
    r = (v - k / 2.0).astype(np.longdouble)
    arg = (np.longdouble(PI) + np.longdouble(1.2246467991473532e-16)) * r
    c, s = np.cos(arg).astype(np.float64), np.sin(arg).astype(np.float64)
    return np.choose(k.astype(np.int64) % 4, [c, -s, -c, s])


def normal_first(seed, stream, counter):
    """The first normal of Philox counter `counter` of stream (seed, stream) (csrc/philox.hpp: normal_pair's z0):
    sqrt(-2 log u1) cos(2 pi u2), u1 = (((r0 << 21) | (r1 >> 11)) + 1) 2^-53 in (0, 1], u2 = ((r2 << 21) | (r3 >> 11)) 2^-53."""
    u64 = np.uint64
    r = toad_ref._words(seed, stream, counter)
    a, b = (r[0] << u64(21)) | (r[1] >> u64(11)), (r[2] << u64(21)) | (r[3] >> u64(11))
    u1, u2 = (a + u64(1)).astype(np.float64) * 2.0 ** -53, b.astype(np.float64) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * _cospi(2.0 * u2)


def philox_draws(seed, stream, first_index, n, n_obs=50):
    """The device's (Z, TH, W), each (n, n_obs): cell (simulation g = first_index + row, time t) reads the counter e =
    (g << 32) | t -- TH and W from stream `stream` exactly as the sampler draws element e, Z the first normal of counter e
    of `stream + 1`."""
    u64 = np.uint64
    g = (np.arange(n, dtype=u64) + u64(first_index))[:, None]
    e = (g << u64(32)) | np.arange(n_obs, dtype=u64)[None, :]
    TH, W = toad_ref.angle_expo(seed, stream, e)
    return normal_first(seed, int(stream) + 1, e), TH, W


def stable_valid(alpha, beta, scale):
    with np.errstate(invalid='ignore'):
        return (alpha > 0) & (alpha <= 2) & (beta >= -1) & (beta <= 1) & (scale >= 0)


def stable_general_step(alpha, beta, loc, scale, TH, W, parameterization='S1'):
    """(x, B): SciPy 1.15's levy_stable.rvs(alpha, beta, loc, scale) on the angle TH and the exponential W, in SciPy's order
    of operations -- _rvs_Z1's alpha1func at alpha == 1, beta0func at beta == 0 (toad_ref.stable_step's expression), otherwise
    `otherwise`; Z scale + loc; rvs's shift X1 + 2 beta gamma log(gamma) / pi at alpha == 1; and for 'S0' the second shift, X1
    - (beta 2 gamma log(gamma) / pi) at alpha == 1, X1 - gamma beta tan(pi alpha / 2) elsewhere.  B is the first-order
    propagation, made as toad_ref.stable_step makes it, of TRANSCENDENTAL_ULP ulp per tan / sin / cos / arctan / log / pow
    call and half an ulp per arithmetic operation (multiplications by 2 and divisions by 2 are exact) through the branch taken
    and both shifts.  Invalid parameters (alpha outside (0, 2], beta outside [-1, 1], scale < 0, NaN) give NaN, B = 0 -- SciPy
    raises for the whole call."""
    if parameterization not in ('S0', 'S1'):
        raise ValueError("parameterization must be 'S0' or 'S1'")
    shape = np.broadcast(alpha, beta, loc, scale, TH, W).shape
    alpha, beta, loc, scale, TH, W = [np.atleast_1d(np.asarray(a, dtype=np.float64))
                                      for a in np.broadcast_arrays(alpha, beta, loc, scale, TH, W)]
    h, t4 = EPS / 2, TRANSCENDENTAL_ULP * EPS
    ab = np.abs
    with np.errstate(all='ignore'):
        ok = stable_valid(alpha, beta, scale)
        one = alpha == 1
        sym = beta == 0
        a = np.where(ok & ~one, alpha, 0.5)
        b = np.where(ok, beta, 0.5)
        tanTH, cosTH, sinTH = np.tan(TH), np.cos(TH), np.sin(TH)
        e_tan, e_cos, e_sin = t4 * ab(tanTH), t4 * ab(cosTH), t4 * ab(sinTH)
        # ---- alpha == 1: 2 / pi ((pi / 2 + bTH) tanTH - beta log((pi / 2 W cosTH) / (pi / 2 + bTH)))
        bTH = b * TH
        s = HALF_PI + bTH
        e_s = h * ab(bTH) + h * ab(s)
        m = s * tanTH
        e_m = ab(s) * e_tan + ab(tanTH) * e_s + h * ab(m)
        hw = HALF_PI * W
        n = hw * cosTH
        e_n = ab(hw) * e_cos + ab(cosTH) * h * ab(hw) + h * ab(n)
        r1 = n / s
        e_r1 = e_n / ab(s) + ab(r1) * e_s / ab(s) + h * ab(r1)
        L = np.log(r1)
        e_L = t4 * ab(L) + e_r1 / ab(r1)
        bl = b * L
        e_bl = ab(b) * e_L + h * ab(bl)
        d = m - bl
        e_d = e_m + e_bl + h * ab(d)
        z1 = TWO_BY_PI * d
        e_z1 = TWO_BY_PI * e_d + h * ab(z1)
        # ---- beta == 0: the symmetric expression (its bound without the closing multiplication by a scale of one)
        z0, B0 = toad_ref.stable_step(a, 1.0, TH, W)
        e_z0 = np.maximum(B0 - h * ab(z0), 0.0)
        # ---- otherwise
        a2 = PI * a / 2
        e_a2 = h * ab(a2)
        tn = np.tan(a2)
        e_tn = t4 * ab(tn) + (1 + tn * tn) * e_a2
        val0 = b * tn
        e_v0 = ab(b) * e_tn + h * ab(val0)
        at = np.arctan(val0)
        e_at = t4 * ab(at) + e_v0 / (1 + val0 * val0)
        th0 = at / a
        e_th0 = e_at / a + h * ab(th0)
        sm = th0 + TH
        e_sm = e_th0 + h * ab(sm)
        arg = a * sm
        e_arg = a * e_sm + h * ab(arg)
        ta = np.tan(arg)
        e_ta = t4 * ab(ta) + (1 + ta * ta) * e_arg
        q1 = cosTH / ta
        e_q1 = e_cos / ab(ta) + ab(q1) * e_ta / ab(ta) + h * ab(q1)
        den = q1 + sinTH
        e_den = e_q1 + e_sin + h * ab(den)
        val3 = W / den
        e_val3 = ab(val3) * (e_den / ab(den) + h)
        aTH = a * TH
        e_aTH = h * ab(aTH)
        ca, sa = np.cos(aTH), np.sin(aTH)
        e_ca = t4 * ab(ca) + ab(sa) * e_aTH
        e_sa = t4 * ab(sa) + ab(ca) * e_aTH
        pr = sa * tanTH
        e_pr = ab(sa) * e_tan + ab(tanTH) * e_sa + h * ab(pr)
        n1 = ca + pr
        e_n1 = e_ca + e_pr + h * ab(n1)
        d1 = ca * tanTH
        e_d1 = ab(ca) * e_tan + ab(tanTH) * e_ca + h * ab(d1)
        d2 = sa - d1
        e_d2 = e_sa + e_d1 + h * ab(d2)
        p2 = val0 * d2
        e_p2 = ab(val0) * e_d2 + ab(d2) * e_v0 + h * ab(p2)
        num = n1 - p2
        e_num = e_n1 + e_p2 + h * ab(num)
        r = num / W
        e_r = e_num / W + h * ab(r)
        ia = 1.0 / a
        pw = r ** ia
        e_pw = ab(pw) * (t4 + ia * e_r / ab(r) + ab(np.log(r)) * h * ia)
        z3 = val3 * pw
        e_z3 = ab(val3) * e_pw + ab(pw) * e_val3 + h * ab(z3)
        Z = np.where(one, z1, np.where(sym, z0, z3))
        e_Z = np.where(one, e_z1, np.where(sym, e_z0, e_z3))
        # ---- rv_continuous.rvs: Z scale + loc
        zs = Z * scale
        x = zs + loc
        B = scale * e_Z + h * ab(zs) + h * ab(x)
        # ---- levy_stable.rvs: the shift of S1 at alpha == 1 and the shift to S0; 2 beta and beta 2 are exact
        lg = np.log(scale)
        sh1 = 2 * b * scale * lg / PI
        e_sh1 = ab(sh1) * (3 * h + t4)
        x1 = x + sh1
        B1 = B + e_sh1 + h * ab(x1)
        x, B = np.where(one, x1, x), np.where(one, B1, B)
        if parameterization == 'S0':
            sh0 = b * 2 * scale * lg / PI
            xa = x - sh0
            Ba = B + ab(sh0) * (3 * h + t4) + h * ab(xa)
            gb = scale * b
            a2f = PI * alpha / 2.0
            tnf = np.tan(a2f)
            shn = gb * tnf
            e_shn = ab(gb) * (t4 * ab(tnf) + (1 + tnf * tnf) * h * ab(a2f)) + 2 * h * ab(shn)
            xn = x - shn
            Bn = B + e_shn + h * ab(xn)
            x, B = np.where(one, xa, xn), np.where(one, Ba, Bn)
        x = np.where(ok, x, np.nan)
        B = np.where(ok & ~np.isnan(x), B, 0.0)
    return x.reshape(shape), B.reshape(shape)


def general_inputs(seed=11):
    """(alpha, beta, loc, scale, TH, W), 30 000 elements, for the sampler's tests on given angles and exponentials: alpha over
    (0.3, 2] and beta over [-1, 1], the exact values alpha 1 and 2 and beta 0 and +-1, TH pushed towards +-pi/2, a block with
    |alpha - 1| from 10^-1 down to 10^-5, and invalid parameters."""
    rs = np.random.RandomState(seed)
    n = 30000
    alpha = rs.uniform(0.3, 2.0, n)
    alpha[alpha <= 0.3] = 2.0
    beta = rs.uniform(-1.0, 1.0, n)
    loc = rs.uniform(-10, 10, n)
    scale = rs.uniform(0, 100, n)
    scale[::97] = 0.0
    TH = rs.uniform(size=n) * PI + (-HALF_PI)
    W = rs.standard_exponential(n)
    alpha[12000:14000], alpha[14000:16000] = 1.0, 2.0
    beta[11000:13000] = 0.0                                # beta == 0 over the range of alpha and at alpha == 1
    beta[13000:13500], beta[13500:14000] = 1.0, -1.0       # ... beta = +-1 at alpha == 1
    beta[15000:15500], beta[15500:16000] = 1.0, -1.0       # ... and at alpha == 2
    beta[16000:17000] = rs.choice([-1.0, 1.0], 1000)       # ... and over the range of alpha
    k = np.arange(17000, 21000)
    TH[k] = rs.choice([-1.0, 1.0], k.size) * (HALF_PI - 10.0 ** -rs.uniform(1, 14, k.size))
    alpha[20000:20500], beta[20500:21000] = 1.0, 0.0       # ... at alpha == 1 and at beta == 0 as well
    # near alpha = 1 the S0 shift cancels Z: from |alpha - 1| of about 10^-4 down the bound passes MASK_RELATIVE for a good part
    # of the elements, so only 60 of the block's 3 000 lie below 10^-3.5 -- the share that is masked stays under MASK_SHARE
    k = np.arange(21000, 24000)
    expo = np.concatenate([rs.uniform(1, 3.5, k.size - 60), rs.uniform(3.5, 5, 60)])
    alpha[k] = 1.0 + rs.choice([-1.0, 1.0], k.size) * 10.0 ** -expo
    bad = np.arange(24000, 24600)
    alpha[bad] = np.resize([-1.0, 0.0, 2.5, np.nan, 2.0000000000000004, np.inf, 1.5, 1.5, 1.5, 1.5, 1.0, 1.5], bad.size)
    beta[bad] = np.resize([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 1.5, -1.0000000000000002, np.nan, 0.5, np.inf, 0.5], bad.size)
    scale[bad] = np.resize([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -1.0, 1.0, np.nan], bad.size)
    return alpha, beta, loc, scale, TH, W


def step_mask(x, B):
    """Elements that are compared: a finite value and a bound within MASK_RELATIVE of |x|."""
    return toad_ref.step_mask(x, B)


def valid_rows(alpha, beta, kappa, eta, mu, phi, sigma, x_0=None):
    """A row is valid when its stable parameters are, sigma >= 0 and no parameter is NaN."""
    ps = [np.asarray(p, dtype=np.float64) for p in (alpha, beta, kappa, eta, mu, phi, sigma)]
    if x_0 is not None:
        ps.append(np.asarray(x_0, dtype=np.float64))
    with np.errstate(invalid='ignore'):
        ok = stable_valid(ps[0], ps[1], ps[2]) & (ps[6] >= 0)
        for p in ps:
            ok = ok & ~np.isnan(p)
    return ok


def log_vol(mu, phi, sigma, Z, x_0=None):
    """x (batch, n_obs): the reference's log_vol on the standard normals Z (batch, n_obs) -- ss.norm.rvs(loc, scale) is
    standard_normal scale + loc: x[0] = Z[0] (sigma / sqrt(1 - min(phi phi, 0.99999))) + mu, or Z[0] sigma + (mu + phi (x_0 -
    mu)) with x_0 given; x[t] = Z[t] sigma + (mu + phi (x[t - 1] - mu))."""
    Z = np.asarray(Z, dtype=np.float64)
    n, n_obs = Z.shape
    mu, phi, sigma = [np.broadcast_to(np.asarray(p, dtype=np.float64).reshape(-1), (n,)) for p in (mu, phi, sigma)]
    x = np.zeros((n, n_obs))
    with np.errstate(all='ignore'):
        if x_0 is None:
            x[:, 0] = Z[:, 0] * (sigma / np.sqrt(1 - np.minimum(phi * phi, PHI_SQUARE_CAP))) + mu
        else:
            x_0 = np.broadcast_to(np.asarray(x_0, dtype=np.float64).reshape(-1), (n,))
            x[:, 0] = Z[:, 0] * sigma + (mu + phi * (x_0 - mu))
        for t in range(1, n_obs):
            x[:, t] = Z[:, t] * sigma + (mu + phi * (x[:, t - 1] - mu))
    return x


def returns(x, v):
    with np.errstate(all='ignore'):
        return np.exp(0.5 * x) * v


def summaries(y, q_kurt=Q_KURT, q_skew=Q_SKEW):
    """(batch, 2): the reference's kurt and skew of y (batch, n_obs) -- np.quantile (method 'linear') as positions and
    NumPy's _lerp on the sorted row; a NaN in the row makes both NaN, as np.quantile does."""
    y = np.asarray(y, dtype=np.float64)
    qk, qs = np.asarray(q_kurt, dtype=np.float64), np.asarray(q_skew, dtype=np.float64)
    out = np.empty((y.shape[0], 2))
    with np.errstate(all='ignore'):
        for b in range(y.shape[0]):
            if np.isnan(y[b]).any():
                out[b] = np.nan
                continue
            v = np.sort(y[b])
            k, s = toad_ref._lerp_quantiles(v, qk), toad_ref._lerp_quantiles(v, qs)
            out[b, 0] = (k[3] - k[0]) / (k[2] - k[1])
            out[b, 1] = ((s[2] - s[1]) - (s[1] - s[0])) / (s[2] - s[0])
    return out


def simulate(alpha, beta, kappa, eta, mu, phi, sigma, Z, TH, W, x_0=None):
    """(x, v, B, y) of the model on given draws; invalid rows are NaN throughout (B = 0 there)."""
    n = Z.shape[0]
    col = lambda p: np.broadcast_to(np.asarray(p, dtype=np.float64).reshape(-1), (n,))[:, None]     # noqa: E731
    ok = np.broadcast_to(valid_rows(alpha, beta, kappa, eta, mu, phi, sigma, x_0).reshape(-1), (n,))
    x = log_vol(mu, phi, sigma, Z, x_0)
    v, B = stable_general_step(col(alpha), col(beta), col(eta), col(kappa), TH, W, 'S0')
    x[~ok], v[~ok], B[~ok] = np.nan, np.nan, 0.0
    return x, v, B, returns(x, v)
