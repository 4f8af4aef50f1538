"""Summary-statistic operations of ELFI's example models on the GPU (bit-identical to NumPy).

Drop-ins for the callables the reference installs with elfi.Summary (a Summary operation is
`fn(*parents) -> array of length batch_size`, also called once on the observed data with a
leading dimension of 1 -- elfi/model/elfi_model.py:915-943, elfi/compiler.py:94-116):

    autocov(x, lag=1)    elfi/examples/ma2.py:40-59
    ss_mean(y)           elfi/examples/gauss.py:142-156
    ss_var(y)            elfi/examples/gauss.py:159-173
    ma2_distance(...)    the fused MA2 path: simulator arithmetic + both summaries + distance
    arch_summaries(...)  the fused ARCH(1) example: series + 17 summaries [+ distance]     elfi/examples/arch.py
    mg1_summaries(...)   the fused M/G/1 example: series, its logarithm, quantiles [+ distance]  elfi/examples/mg1.py
    lorenz_summaries(...)  the fused stochastic Lorenz-96 example: series + 6 summaries [+ distance]   elfi/examples/lorenz.py
    gnk_summaries(...), bignk_summaries(...)  the fused g-and-k examples: series, order statistics, octiles, robust
                         statistics [+ distance]                                      elfi/examples/gnk.py, bignk.py
    ricker_summaries(...)  the fused Ricker example: stock, Poisson counts, Mean / Var / #0 [+ distance]  elfi/examples/ricker.py
    poisson(lam, ...)    Poisson variates from the library's counter-based generator (csrc/poisson.hpp)
    toad_summaries(...)  the fused toad movement example: alpha-stable steps, refuge chain, a workgroup sort per lag,
                         48 summaries                                                  elfi/examples/toad.py
    levy_stable(alpha, ...)  symmetric alpha-stable variates from the library's counter-based generator (csrc/stable.hpp)
    sv_summaries(...)    the fused alpha-stable stochastic-volatility example: AR(1) log-volatilities, skewed stable shocks,
                         returns, a workgroup sort, kurt and skew               elfi/examples/stochastic_volatility_model.py
    levy_stable_general(alpha, beta, ...)  alpha-stable variates with skewness and location, S1 or S0 (csrc/stable.hpp)
    lotka_volterra_summaries(...)  the stochastic Lotka-Volterra example: Gillespie simulation, observations, 9 summaries
                         [+ distance]                                             elfi/examples/lotka_volterra.py
    daycare_summaries(...)  the day-care-centre transmission example: Gillespie simulation of every centre, 4 summaries per
                         centre [+ distance]; daycare_distance(...) its sorted L1 distance      elfi/examples/daycare.py
    scratch_assay_summaries(...)  the scratch-assay example: the lattice walk of up to 1024 cells, its 145 summaries
                                                                                  elfi/examples/scratch_assay.py
    bdm_clusters(...)    the birth-death-mutation example: the jump chain of up to 4096 clusters, T1, T2 [+ distance] -- no
                         executable, no files                                          elfi/examples/bdm.py, cpp/bdm.cpp
    ar1_series(...)      the AR(1) example: the series [+ the euclidean distance on it]          elfi/examples/ar1.py

    S1 = elfi.Summary(elfi_amd.autocov, Y);  S2 = elfi.Summary(elfi_amd.autocov, Y, 2)

Module-level functions (picklable), plain data in, NumPy arrays out; the arithmetic runs in
libelfihip.so (csrc/summaries.hip, csrc/series.hip, csrc/lorenz.hip, csrc/gnk.hip) with NumPy's pairwise summation order.  No CPU
fallback.
"""
import ctypes as C

import numpy as np

from . import _lib

MEAN, VAR, AUTOCOV = 0, 1, 2


def _rows(x):
    x = np.atleast_2d(np.asarray(x))
    if x.ndim != 2:
        raise ValueError('summary input must be at most 2-dimensional (batch, n_obs)')
    if x.dtype != np.float64 or x.strides[1] != 8 or x.strides[0] % 8 or x.strides[0] < 8 * x.shape[1]:
        x = np.ascontiguousarray(x, dtype=np.float64)
    return x


def _row_summary(kind, x, lag=0, ctx=None):
    x = _rows(x)
    n, L = x.shape
    out = np.empty(n, dtype=np.float64)
    ldx = x.strides[0] // 8 if n > 1 else L
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_row_summary", kind, _lib.ptr(x), n, L, ldx, int(lag), _lib.ptr(out))
    return out


def autocov(x, lag=1):
    """Autocovariance at `lag` (mean assumed zero), per row: np.mean(x[:, lag:] * x[:, :-lag], axis=1)."""
    x = _rows(x)
    if not 1 <= int(lag) < x.shape[1]:
        raise ValueError('lag must be in [1, n_obs)')
    return _row_summary(AUTOCOV, x, lag)


def ss_mean(y):
    """np.mean(y, axis=1)."""
    return _row_summary(MEAN, y)


def ss_var(y):
    """np.var(y, axis=1) (ddof = 0)."""
    return _row_summary(VAR, y)


def ma2_distance(w, t1, t2, observed, ctx=None):
    """Fused MA2 path.  w: (batch, n_obs + 2) white noise as `random_state.randn(batch, n_obs + 2)`
    draws it (elfi/examples/ma2.py:35); t1, t2: (batch,) or scalars; observed: the two observed
    summaries (autocov(y_obs, 1), autocov(y_obs, 2)).  Returns (S1, S2, d), each (batch,)."""
    w = _rows(w)
    n, L = w.shape
    if L < 5:
        raise ValueError('need n_obs >= 3')
    w = np.ascontiguousarray(w)
    t1 = np.ascontiguousarray(np.broadcast_to(np.asarray(t1, dtype=np.float64).reshape(-1), (n,)))
    t2 = np.ascontiguousarray(np.broadcast_to(np.asarray(t2, dtype=np.float64).reshape(-1), (n,)))
    o = np.asarray(observed, dtype=np.float64).reshape(-1)
    if o.shape[0] != 2:
        raise ValueError('observed must hold the two observed summaries')
    S1, S2, D = np.empty(n), np.empty(n), np.empty(n)
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_ma2_distance", _lib.ptr(w), n, L - 2, _lib.ptr(t1), _lib.ptr(t2), C.c_double(o[0]),
             C.c_double(o[1]), _lib.ptr(S1), _lib.ptr(S2), _lib.ptr(D))
    return S1, S2, _lib.remember_kept(D, ctx)


def ma2_draw_distance(t1, t2, observed, n_obs=100, seed=0, stream=0, ctx=None):
    """The whole MA2 example as ONE device operation (elfi/examples/ma2.py:11-59 + Distance('euclidean', S1, S2)): the
    white noise is drawn inside the kernel (Philox4x32-10 keyed by `seed`, counter stream `stream`), the series never
    exists in memory.  t1, t2: (batch,); observed: the two observed summaries.  Returns (S1, S2, d), each (batch,)."""
    t1 = np.asarray(t1, dtype=np.float64).reshape(-1)
    t2 = np.asarray(t2, dtype=np.float64).reshape(-1)
    n = max(t1.shape[0], t2.shape[0])
    t1 = np.ascontiguousarray(np.broadcast_to(t1, (n,)))
    t2 = np.ascontiguousarray(np.broadcast_to(t2, (n,)))
    o = np.asarray(observed, dtype=np.float64).reshape(-1)
    if o.shape[0] != 2:
        raise ValueError('observed must hold the two observed summaries')
    if int(n_obs) < 3:
        raise ValueError('need n_obs >= 3')
    S1, S2, D = np.empty(n), np.empty(n), np.empty(n)
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_ma2_draw_distance", C.c_uint64(int(seed)), C.c_uint64(int(stream)), n, int(n_obs), _lib.ptr(t1),
             _lib.ptr(t2), C.c_double(o[0]), C.c_double(o[1]), _lib.ptr(S1), _lib.ptr(S2), _lib.ptr(D))
    return S1, S2, _lib.remember_kept(D, ctx)


def gauss_distance(mu, sigma, observed, n_obs=50, z=None, seed=0, stream=0, return_y=False, ctx=None):
    """Fused Gaussian example (elfi/examples/gauss.py: gauss -> ss_mean, ss_var -> euclidean distance).

    mu, sigma: (batch,) or scalars; observed: the two observed summaries (ss_mean(y_obs), ss_var(y_obs)).
    z: (batch, n_obs) standard normals as `random_state.standard_normal((batch, n_obs))` draws them -- what
    ss.norm.rvs(loc=mu, scale=sigma, size=(batch, n_obs), random_state=...) consumes (gauss.py:31-33) -- for results
    bit-identical to the reference; z=None draws on the device (Philox4x32-10 keyed by `seed`, stream `stream`), in
    which case the batch size comes from mu / sigma.  Returns (ss_mean, ss_var, d) [, y]."""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if z is not None:
        z = np.ascontiguousarray(_rows(z))
        n, n_obs = z.shape
    else:
        n = max(mu.shape[0], sigma.shape[0])
        n_obs = int(n_obs)
    mu = np.ascontiguousarray(np.broadcast_to(mu, (n,)))
    sigma = np.ascontiguousarray(np.broadcast_to(sigma, (n,)))
    o = np.asarray(observed, dtype=np.float64).reshape(-1)
    if o.shape[0] != 2:
        raise ValueError('observed must hold the two observed summaries')
    S1, S2, D = np.empty(n), np.empty(n), np.empty(n)
    Y = np.empty((n, n_obs)) if return_y else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_gauss_distance", _lib.ptr(z), C.c_uint64(int(seed)), C.c_uint64(int(stream)), n, n_obs,
             _lib.ptr(mu), _lib.ptr(sigma), C.c_double(o[0]), C.c_double(o[1]), _lib.ptr(Y), _lib.ptr(S1), _lib.ptr(S2),
             _lib.ptr(D))
    _lib.remember_kept(D, ctx)
    return (S1, S2, D, Y) if return_y else (S1, S2, D)


# ---- the time-series example models (csrc/series.hip) ---------------------------------------------------------------
SERIES_MAX_OBS = 2048       # include/elfihip.h: ELFIHIP_SERIES_MAX_OBS (a simulation keeps its series in LDS)
ARCH_MAX_LAGS = 8
MG1_MAX_QUANTILES = 64


def _params(n, *ts):
    out = []
    for t in ts:
        t = np.asarray(t, dtype=np.float64).reshape(-1)
        if t.shape[0] not in (1, n):
            raise ValueError('parameters must be scalars or hold one value per simulation (%d)' % n)
        out.append(np.ascontiguousarray(np.broadcast_to(t, (n,))))
    return out


def _batch_of(*ts):
    return max(np.asarray(t).reshape(-1).shape[0] for t in ts)


def arch_n_summaries(n_lags=5):
    return 2 + n_lags + n_lags * (n_lags - 1) // 2


def arch_summaries(t1, t2, n_obs=100, n_lags=5, noise=None, seed=0, stream=0, observed=None, return_series=False,
                   ctx=None):
    """The ARCH(1) example (elfi/examples/arch.py) as ONE device operation: the series e_i = xi_i sqrt(0.2 + t2 e_{i-1}^2),
    y_i = t1 y_{i-1} + e_i and its 2 + L + L (L - 1) / 2 summaries -- sample_mean, sample_variance, autocorr at lags 1 .. L =
    n_lags, pairwise_autocorr(i, j), i < j -- in the reference's column order MU, VAR, AC_1 .., PW_1_2 ...

    t1, t2: (batch,) or scalars.  noise: (batch, n_obs + 2) standard normals (for the n_obs given; any other shape is a
    ValueError), columns 0 .. n_obs what the reference draws
    as `normal(size=(batch, n_obs + 1))` and the last column its `normal(size=batch)` -- results bit-identical to the
    reference's NumPy; noise=None draws on the device (Philox4x32-10 keyed by `seed`, counter stream `stream`).
    observed: the observed summaries; with them the euclidean distance is returned too.
    Returns S (batch, m) [, series (batch, n_obs)] [, d (batch,)]."""
    n_obs, n_lags = int(n_obs), int(n_lags)
    if not 1 <= n_lags <= ARCH_MAX_LAGS:
        raise ValueError('n_lags must be in [1, %d]' % ARCH_MAX_LAGS)
    if noise is not None:
        noise = np.asarray(noise)
        if noise.ndim != 2 or noise.shape[1] != n_obs + 2:
            raise ValueError('noise must be (batch, n_obs + 2) = (batch, %d)' % (n_obs + 2))
    if n_obs < n_lags + 2:
        raise ValueError('need n_obs >= n_lags + 2')
    if n_obs > SERIES_MAX_OBS:
        raise ValueError('series of at most %d observations' % SERIES_MAX_OBS)
    n = noise.shape[0] if noise is not None else _batch_of(t1, t2)
    t1, t2 = _params(n, t1, t2)
    m = arch_n_summaries(n_lags)
    obs = None
    if observed is not None:
        obs = np.ascontiguousarray(np.asarray(observed, dtype=np.float64).reshape(-1))
        if obs.shape[0] != m:
            raise ValueError('observed must hold the %d observed summaries' % m)
    if noise is not None:
        noise = np.ascontiguousarray(noise, dtype=np.float64)
    S = np.empty((n, m))
    Y = np.empty((n, n_obs)) if return_series else None
    D = np.empty(n) if obs is not None else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_arch_summaries", _lib.ptr(noise), C.c_uint64(int(seed)), C.c_uint64(int(stream)), n, n_obs, n_lags,
             _lib.ptr(t1), _lib.ptr(t2), _lib.ptr(obs), _lib.ptr(S), _lib.ptr(Y), _lib.ptr(D))
    return tuple(a for a in (S, Y, D) if a is not None) if (return_series or obs is not None) else S


def ar1_series(phi, n_obs=200, noise=None, seed=0, stream=0, observed=None, ctx=None):
    """The AR(1) example (elfi/examples/ar1.py) as ONE device operation: x_0 = 0, x_i = phi x_{i-1} + w_i, i = 1 .. n_obs, the
    product rounded before the sum as NumPy does.

    phi: (batch,) or a scalar; NaN and infinite values propagate as NumPy's do.  noise: (batch, n_obs + 1) standard normals,
    the reference's `randn(batch, n_obs + 1)` with its unused column 0 (any other shape is a ValueError) -- the series is then
    bit-identical to the reference's; noise=None draws on the device (Philox4x32-10 keyed by `seed`, counter stream `stream`:
    element e of the row-major matrix is normal number e).  observed: the observed series (n_obs values); with it the
    euclidean distance of every row, bit-identical to elfi_amd's row distance on the series, is returned too.
    Returns X (batch, n_obs) [, d (batch,)]."""
    n_obs = int(n_obs)
    if not 1 <= n_obs <= SERIES_MAX_OBS:
        raise ValueError('n_obs must be in [1, %d]' % SERIES_MAX_OBS)
    if noise is not None:
        noise = np.asarray(noise)
        if noise.ndim != 2 or noise.shape[1] != n_obs + 1:
            raise ValueError('noise must be (batch, n_obs + 1) = (batch, %d)' % (n_obs + 1))
    n = noise.shape[0] if noise is not None else _batch_of(phi)
    if n < 1:
        raise ValueError('need at least one simulation')
    phi, = _params(n, phi)
    obs = None
    if observed is not None:
        obs = np.ascontiguousarray(np.asarray(observed, dtype=np.float64).reshape(-1))
        if obs.shape[0] != n_obs:
            raise ValueError('observed must hold the %d observed values' % n_obs)
    if noise is not None:
        noise = np.ascontiguousarray(noise, dtype=np.float64)
    X = np.empty((n, n_obs))
    D = np.empty(n) if obs is not None else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_ar1_series", _lib.ptr(noise), C.c_uint64(int(seed)), C.c_uint64(int(stream)), n, n_obs, _lib.ptr(phi),
             _lib.ptr(obs), _lib.ptr(X), _lib.ptr(D))
    return (X, D) if D is not None else X


def quantile_positions(q, n):
    """np.quantile(method='linear') on n sorted values, as positions: (lo, hi, t) -- the two neighbours of the virtual index
    (n - 1) q and the interpolation weight (NumPy's _get_indexes / _get_gamma: at the upper end both neighbours are the last
    element, which NumPy names -1, and the weight is measured from that name)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    virt = (n - 1) * q
    prev = np.floor(virt)
    nxt = prev + 1
    above = virt >= n - 1
    prev[above], nxt[above] = -1, -1
    below = virt < 0
    prev[below], nxt[below] = 0, 0
    t = virt - prev
    return (prev.astype(np.int64) % n).astype(np.int32), (nxt.astype(np.int64) % n).astype(np.int32), t


def mg1_summaries(t1, t2, t3, n_obs=50, q=None, draws=None, seed=0, stream=0, observed=None, w=None, return_series=False,
                  return_draws=False, ctx=None):
    """The M/G/1 queue example (elfi/examples/mg1.py) as ONE device operation: inter-departure times y_i = U_i + max(0,
    sum_w - sum_x) from arrivals every (1 / t3) E and service times t1 + (t2 - t1) V, their logarithm (log_identity) and
    the quantiles np.quantile(y, q, axis=1).T (default q: 10 equidistant in [0, 1], the example's).

    draws: (E, V), each (batch, n_obs) -- standard exponentials and uniforms in [0, 1), what the reference consumes as
    standard_exponential((n_obs, batch)).T and random_sample((n_obs, batch)).T: series and quantiles bit-identical to the
    reference's NumPy; draws=None draws on the device (`seed`; counter streams `stream` and `stream + 1`).
    observed: the observed quantiles, w: weights; with `observed` the (weighted) euclidean distance is returned too.
    Returns log_y (batch, n_obs), quantiles (batch, nq) [, y] [, E, V] [, d]."""
    n_obs = int(n_obs)
    q = np.linspace(0, 1, 10) if q is None else np.asarray(q, dtype=np.float64).reshape(-1)
    if not 1 <= q.shape[0] <= MG1_MAX_QUANTILES:
        raise ValueError('1 to %d quantiles' % MG1_MAX_QUANTILES)
    if not np.all((q >= 0) & (q <= 1)):
        raise ValueError('Quantiles must be in the range [0, 1]')
    E = V = None
    if draws is not None:
        E, V = [np.asarray(a) for a in draws]
        if E.ndim != 2 or E.shape != V.shape or E.shape[1] != n_obs:
            raise ValueError('draws must be two (batch, n_obs) = (batch, %d) arrays: exponentials and uniforms' % n_obs)
    if n_obs < 2:
        raise ValueError('need n_obs >= 2')
    if n_obs > SERIES_MAX_OBS:
        raise ValueError('series of at most %d observations' % SERIES_MAX_OBS)
    if w is not None and observed is None:
        raise ValueError('weights need the observed quantiles')
    nq = q.shape[0]
    obs = None
    if observed is not None:
        obs = np.ascontiguousarray(np.asarray(observed, dtype=np.float64).reshape(-1))
        if obs.shape[0] != nq:
            raise ValueError('observed must hold the %d observed quantiles' % nq)
    if w is not None:
        w = np.ascontiguousarray(np.asarray(w, dtype=np.float64).reshape(-1))
        if w.shape[0] != nq:
            raise ValueError('w must hold one weight per quantile (%d)' % nq)
    n = E.shape[0] if E is not None else _batch_of(t1, t2, t3)
    t1, t2, t3 = _params(n, t1, t2, t3)
    if E is not None:
        E, V = np.ascontiguousarray(E, dtype=np.float64), np.ascontiguousarray(V, dtype=np.float64)
    lo, hi, t = [np.ascontiguousarray(a) for a in quantile_positions(q, n_obs)]
    logY, Q = np.empty((n, n_obs)), np.empty((n, nq))
    Y = np.empty((n, n_obs)) if return_series else None
    Eo = np.empty((n, n_obs)) if return_draws else None
    Vo = np.empty((n, n_obs)) if return_draws else None
    D = np.empty(n) if obs is not None else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_mg1_summaries", _lib.ptr(E), _lib.ptr(V), C.c_uint64(int(seed)), C.c_uint64(int(stream)), n, n_obs,
             _lib.ptr(t1), _lib.ptr(t2), _lib.ptr(t3), nq, _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(t), _lib.ptr(obs),
             _lib.ptr(w), _lib.ptr(logY), _lib.ptr(Q), _lib.ptr(Y), _lib.ptr(Eo), _lib.ptr(Vo), _lib.ptr(D))
    return tuple(a for a in (logY, Q, Y, Eo, Vo, D) if a is not None)


# ---- the stochastic Lorenz-96 example model (csrc/lorenz.hip) -------------------------------------------------------
LORENZ_MAX_VARS = 64        # include/elfihip.h: ELFIHIP_LORENZ_MAX_VARS (a variable per lane)
LORENZ_MAX_TERMS = 8192     # ELFIHIP_LORENZ_MAX_TERMS (n_timestep * n_obs: NumPy's reduction buffer)
LORENZ_NAMES = ('Mean', 'Var', 'Autocov', 'Cov', 'CrosscovPrev', 'CrosscovNext')


def lorenz_summaries(theta1, theta2, initial_state, f=10., phi=0.984, n_obs=40, n_timestep=160, total_duration=4,
                     noise=None, seed=0, stream=0, observed=None, return_series=False, ctx=None):
    """The stochastic Lorenz-96 forecast example (elfi/examples/lorenz.py) as ONE device operation: n_obs cyclically coupled
    variables stepped n_timestep - 1 times by fourth-order Runge-Kutta under an AR(1) forcing eta = phi eta + e sqrt(1 -
    phi^2), and the six summaries of the (n_timestep, n_obs) series in the reference's order Mean, Var, Autocov, Cov,
    CrosscovPrev, CrosscovNext.

    theta1, theta2: (batch,) or scalars.  initial_state: (n_obs,) shared by all simulations, or (batch, n_obs).
    noise: (batch, n_timestep - 1, n_obs) standard normals, what the reference draws as `normal(0, 1, (batch, n_obs))` once
    per step, stacked along axis 1 -- series and summaries bit-identical to the reference's NumPy; noise=None draws on the
    device (Philox4x32-10 keyed by `seed`, counter stream `stream`).  4 <= n_obs <= 64, n_timestep >= 2, n_timestep * n_obs
    <= 8192.  observed: the six observed summaries; with them the euclidean distance is returned too.
    Returns S (batch, 6) [, series (batch, n_timestep, n_obs)] [, d (batch,)]."""
    n_obs, n_timestep = int(n_obs), int(n_timestep)
    if not 4 <= n_obs <= LORENZ_MAX_VARS:
        raise ValueError('n_obs must be in [4, %d]' % LORENZ_MAX_VARS)
    if n_timestep < 2:
        raise ValueError('need n_timestep >= 2')
    if n_timestep * n_obs > LORENZ_MAX_TERMS:
        raise ValueError('n_timestep * n_obs must be at most %d' % LORENZ_MAX_TERMS)
    if not abs(float(phi)) <= 1.0:
        raise ValueError('phi must be in [-1, 1]')
    if noise is not None:
        noise = np.asarray(noise)
        if noise.ndim != 3 or noise.shape[1:] != (n_timestep - 1, n_obs):
            raise ValueError('noise must be (batch, n_timestep - 1, n_obs) = (batch, %d, %d)' % (n_timestep - 1, n_obs))
    y0 = np.asarray(initial_state, dtype=np.float64)
    if y0.ndim not in (1, 2) or y0.shape[-1] != n_obs:
        raise ValueError('initial_state must be (n_obs,) or (batch, n_obs) with n_obs = %d' % n_obs)
    n = noise.shape[0] if noise is not None else (y0.shape[0] if y0.ndim == 2 else _batch_of(theta1, theta2))
    if y0.ndim == 2 and y0.shape[0] != n:
        raise ValueError('initial_state must hold one row per simulation (%d)' % n)
    theta1, theta2 = _params(n, theta1, theta2)
    obs = None
    if observed is not None:
        obs = np.ascontiguousarray(np.asarray(observed, dtype=np.float64).reshape(-1))
        if obs.shape[0] != 6:
            raise ValueError('observed must hold the 6 observed summaries')
    y0 = np.ascontiguousarray(y0)
    if noise is not None:
        noise = np.ascontiguousarray(noise, dtype=np.float64)
    c = float(np.sqrt(1 - pow(phi, 2)))          # lorenz.py:157, as Python computes it
    h = total_duration / n_timestep              # lorenz.py:148
    S = np.empty((n, 6))
    Y = np.empty((n, n_timestep, n_obs)) if return_series else None
    D = np.empty(n) if obs is not None else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_lorenz_summaries", _lib.ptr(noise), C.c_uint64(int(seed)), C.c_uint64(int(stream)), n, n_obs, n_timestep,
             _lib.ptr(theta1), _lib.ptr(theta2), C.c_double(f), C.c_double(c), C.c_double(phi), C.c_double(h), _lib.ptr(y0),
             int(y0.ndim == 2), _lib.ptr(obs), _lib.ptr(S), _lib.ptr(Y), _lib.ptr(D))
    return tuple(a for a in (S, Y, D) if a is not None) if (return_series or obs is not None) else S


# ---- the g-and-k example models (csrc/gnk.hip) ----------------------------------------------------------------------
GNK_SUMMARIES = ('order', 'sorted', 'octile', 'robust')     # include/elfihip.h: ELFIHIP_GNK_ORDER, _SORTED, _OCTILE, _ROBUST
GNK_OCTILES = np.linspace(12.5, 87.5, 7)                    # gnk.py:207


def gnk_summary_length(name, n_obs, dim=1):
    """Values per simulation of the summary `name`."""
    return {'order': n_obs * dim, 'sorted': n_obs * dim, 'octile': 7 * dim, 'robust': 4 * dim}[name]


def _gnk_call(params, dim, c, n_obs, z, seed, stream, summary, observed, return_series, return_draws, ctx):
    n_obs = int(n_obs)
    single = isinstance(summary, str)
    names = (summary,) if single else (tuple(summary) if isinstance(summary, (tuple, list)) else ())
    if not names or any(not isinstance(s, str) or s not in GNK_SUMMARIES for s in names):
        raise ValueError('summary must be one of %s, or a tuple of them' % (GNK_SUMMARIES,))
    shape = (n_obs,) if dim == 1 else (n_obs, 2)
    if z is not None:
        z = np.asarray(z)
        if z.ndim != 1 + len(shape) or z.shape[1:] != shape:
            raise ValueError('z must be (batch,%s)' % ''.join(' %d,' % s for s in shape)[:-1])
    if n_obs < 2:
        raise ValueError('need n_obs >= 2')
    if n_obs * dim > SERIES_MAX_OBS:
        raise ValueError('series of at most %d values (n_obs * %d)' % (SERIES_MAX_OBS, dim))
    n = z.shape[0] if z is not None else _batch_of(*params)
    P = np.ascontiguousarray(np.column_stack(_params(n, *params)))
    if dim == 2 and not np.all(np.abs(P[:, 8]) <= 1.0):
        raise ValueError('rho must be in [-1, 1]')
    obs = None
    if observed is not None:
        m = gnk_summary_length(names[0], n_obs, dim)
        obs = np.ascontiguousarray(np.asarray(observed, dtype=np.float64).reshape(-1))
        if obs.shape[0] != m:
            raise ValueError('observed must hold the %d values of the summary %r' % (m, names[0]))
    if z is not None:
        z = np.ascontiguousarray(z, dtype=np.float64)
    lo, hi, t = [np.ascontiguousarray(a) for a in quantile_positions(np.true_divide(GNK_OCTILES, 100), n_obs)]
    L = n_obs * dim
    Y = np.empty((n, L)) if (return_series or 'order' in names) else None
    Zo = np.empty((n,) + shape) if return_draws else None
    Ys = np.empty((n, L)) if 'sorted' in names else None
    O = np.empty((n, 7 * dim)) if 'octile' in names else None
    R = np.empty((n, 4 * dim)) if 'robust' in names else None
    D = np.empty(n) if obs is not None else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_gnk_summaries", _lib.ptr(z), C.c_uint64(int(seed)), C.c_uint64(int(stream)), n, n_obs, dim,
             _lib.ptr(P), C.c_double(c), _lib.ptr(lo), _lib.ptr(hi), _lib.ptr(t), _lib.ptr(obs),
             GNK_SUMMARIES.index(names[0]), _lib.ptr(Y), _lib.ptr(Zo), _lib.ptr(Ys), _lib.ptr(O), _lib.ptr(R), _lib.ptr(D))
    by_name = dict(order=Y, sorted=Ys, octile=O, robust=R)
    out = [by_name[s] for s in names]
    if return_series:
        out.append(Y.reshape((n,) + shape))
    if return_draws:
        out.append(Zo)
    if D is not None:
        out.append(D)
    return out[0] if (single and len(out) == 1) else tuple(out)


def gnk_summaries(A, B, g, k, c=0.8, n_obs=50, z=None, seed=0, stream=0, summary='robust', observed=None,
                  return_series=False, return_draws=False, ctx=None):
    """The univariate g-and-k example (elfi/examples/gnk.py) as ONE device operation: the series y = A + B (1 + c (1 -
    exp(-g z)) / (1 + exp(-g z))) (1 + z^2)^k z in the reference's order of operations, and its summaries.

    A, B, g, k: (batch,) or scalars.  z: (batch, n_obs) standard normals, what the reference draws as
    ss.norm.rvs(size=(batch, n_obs)); z=None draws on the device (Philox4x32-10 keyed by `seed`, counter stream `stream`:
    element e is normal number e of that stream).  The series passes through the device's exp and pow and is within a few
    units eps (|A| + |y - A|) of the reference's; every summary is NumPy's bit for bit on the device's series.
    summary: 'order' (the series as it is: the reference's ss_order, whose np.sort runs along the last axis), 'sorted'
    (np.sort(y, axis=1): true order statistics, not a reference summary), 'octile' (ss_octile, 7 values), 'robust'
    (ss_robust, 4 values), or a tuple of them.  observed: the observed values of the FIRST summary named; with them the
    euclidean distance on that summary is returned too (HipDistance's bits; euclidean_multiss up to its order of summation).
    Returns the summaries in the order asked, each (batch, m) [, series (batch, n_obs)] [, draws (batch, n_obs)] [, d
    (batch,)] -- the bare array when `summary` is one name and nothing else is asked for, else a tuple."""
    return _gnk_call((A, B, g, k), 1, float(c), n_obs, z, seed, stream, summary, observed, return_series, return_draws, ctx)


def bignk_summaries(A1, A2, B1, B2, g1, g2, k1, k2, rho, c=0.8, n_obs=150, z=None, seed=0, stream=0, summary='robust',
                    observed=None, return_series=False, return_draws=False, ctx=None):
    """The bivariate g-and-k example (elfi/examples/bignk.py) as ONE device operation: per simulation n_obs pairs of
    normals with correlation rho, the g-and-k quantile function per dimension, and the summaries of gnk_summaries per
    dimension, stacked as the reference stacks them: 'octile' (batch, 14) = [E1_d0, E1_d1, E2_d0, ...], 'robust' (batch, 8)
    = [A_d0, A_d1, B_d0, ...]; 'order' and 'sorted' (batch, 2 n_obs) are (n_obs, 2) row-major per simulation.

    z: (batch, n_obs, 2) ALREADY correlated normals, as the reference holds them (multivariate_normal.rvs(cov=[[1, rho],
    [rho, 1]], size=n_obs) per simulation); z=None draws on the device: the pair (e0, e1) of an observation -- normals 2 j
    and 2 j + 1 of (seed, stream) -- becomes z0 = e0, z1 = rho e0 + sqrt(1 - rho^2) e1, the distribution of the reference's
    draws, not their bits.  |rho| <= 1.  Series and draws come back as (batch, n_obs, 2).  Otherwise as gnk_summaries."""
    return _gnk_call((A1, A2, B1, B2, g1, g2, k1, k2, rho), 2, float(c), n_obs, z, seed, stream, summary, observed,
                     return_series, return_draws, ctx)


# ---- Poisson variates and the Ricker example model (csrc/poisson.hpp, csrc/series.hip) ------------------------------
RICKER_DISTANCES = ('chi_squared', 'euclidean_mean')     # include/elfihip.h: ELFIHIP_RICKER_CHI2, _EUCLID_MEAN
RICKER_NAMES = ('Mean', 'Var', '#0')


def poisson(lam, seed=0, stream=0, ctx=None):
    """Poisson variates with intensities `lam` from the library's counter-based generator, in the shape of `lam`, as
    float64: element e of the flattened array is a fixed function of lam[e] and of Philox counter e of the streams (seed,
    stream), (seed, stream + 1), ... -- inversion below 10, Hoermann's transformed rejection (NumPy's legacy algorithm) from
    10 on, one stream per attempt; a fused kernel that draws element e itself gets the same number.  lam == 0 gives 0.
    A NaN, negative or above-2^53 intensity gives NaN for that element (RandomState.poisson raises ValueError for the
    whole batch instead)."""
    lam = np.asarray(lam, dtype=np.float64)
    flat = np.ascontiguousarray(lam.reshape(-1))
    out = np.empty(flat.shape[0])
    if flat.shape[0] == 0:
        return out.reshape(lam.shape)
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_poisson", C.c_uint64(int(seed)), C.c_uint64(int(stream)), flat.shape[0], _lib.ptr(flat), _lib.ptr(out))
    return out.reshape(lam.shape)


def ricker_summaries(log_rate, std=None, scale=None, stock_init=1., n_obs=50, noise=None, seed=0, stream=0, observed=None,
                     distance='chi_squared', return_series=False, return_stock=False, return_draws=False, ctx=None):
    """The Ricker example (elfi/examples/ricker.py) as ONE device operation: the stock s_i = s_{i-1} exp(log_rate - s_{i-1} +
    std z_i), s_0 = stock_init, its Poisson observation y_i ~ Poisson(scale s_i) and the summaries Mean = np.mean(y, axis=1),
    Var = np.var(y, axis=1), #0 = the number of zero observations.  std = scale = None is the deterministic model: y_0 =
    stock_init, y_i = y_{i-1} exp(log_rate - y_{i-1}), no draws (both are given or both None).

    log_rate, std, scale: (batch,) or scalars; stock_init a scalar.  noise: (batch, n_obs) standard normals, the
    reference's randn(batch) of step i in column i - 1 (any other shape is a ValueError); noise=None draws on the device
    (Philox4x32-10 keyed by `seed`, counter stream `stream`).  The Poisson counts are always the device's: element e =
    row * n_obs + i - 1 is elfi_amd.poisson's element e on the streams from `stream + 1` on.  A stock that has underflowed
    to 0 is observed as 0, one that has overflowed as NaN (the reference raises ValueError for the whole batch).
    observed: the 3 observed summaries; with them the distance is returned too -- 'chi_squared' (the reference's: sum((S -
    obs)^2 / obs)) or 'euclidean_mean' (euclidean on the Mean column alone, the deterministic model's d).
    Returns S (batch, 3) [, series (batch, n_obs)] [, stock (batch, n_obs)] [, normals (batch, n_obs)] [, d (batch,)] -- the
    bare array when nothing else is asked for."""
    n_obs = int(n_obs)
    if (std is None) != (scale is None):
        raise ValueError('std and scale are given together (the stochastic model) or not at all (the deterministic one)')
    stochastic = std is not None
    if distance not in RICKER_DISTANCES:
        raise ValueError('distance must be one of %s' % (RICKER_DISTANCES,))
    if not 1 <= n_obs <= SERIES_MAX_OBS:
        raise ValueError('n_obs must be in [1, %d]' % SERIES_MAX_OBS)
    if noise is not None:
        if not stochastic:
            raise ValueError('the deterministic model takes no noise')
        noise = np.asarray(noise)
        if noise.ndim != 2 or noise.shape[1] != n_obs:
            raise ValueError('noise must be (batch, n_obs) = (batch, %d)' % n_obs)
    if return_draws and not stochastic:
        raise ValueError('the deterministic model makes no draws')
    params = (log_rate, std, scale) if stochastic else (log_rate,)
    n = noise.shape[0] if noise is not None else _batch_of(*params)
    if n < 1:
        raise ValueError('need at least one simulation')
    params = _params(n, *params)
    obs = None
    if observed is not None:
        obs = np.ascontiguousarray(np.asarray(observed, dtype=np.float64).reshape(-1))
        if obs.shape[0] != 3:
            raise ValueError('observed must hold the 3 observed summaries Mean, Var, #0')
    if noise is not None:
        noise = np.ascontiguousarray(noise, dtype=np.float64)
    S = np.empty((n, 3))
    Y = np.empty((n, n_obs)) if return_series else None
    St = np.empty((n, n_obs)) if return_stock else None
    Zo = np.empty((n, n_obs)) if return_draws else None
    D = np.empty(n) if obs is not None else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_ricker_summaries", _lib.ptr(noise), C.c_uint64(int(seed)), C.c_uint64(int(stream)), n, n_obs,
             _lib.ptr(params[0]), _lib.ptr(params[1]) if stochastic else None, _lib.ptr(params[2]) if stochastic else None,
             C.c_double(float(stock_init)), _lib.ptr(obs), RICKER_DISTANCES.index(distance), _lib.ptr(S), _lib.ptr(Y),
             _lib.ptr(St), _lib.ptr(Zo), _lib.ptr(D))
    out = tuple(a for a in (S, Y, St, Zo, D) if a is not None)
    return out if len(out) > 1 else S


# ---- the stochastic Lotka-Volterra example model (csrc/gillespie.hip) -------------------------------------------------
LV_NAMES = ('prey_mean', 'pred_mean', 'prey_log_var', 'pred_log_var', 'prey_autocorr_1', 'pred_autocorr_1',
            'prey_autocorr_2', 'pred_autocorr_2', 'crosscorr')
LV_MAX_EVENTS = 1 << 30                                   # include/elfihip.h: ELFIHIP_LV_MAX_EVENTS
LV_STATUS = ('reached_end', 'extinct', 'out_of_events', 'invalid')     # ELFIHIP_LV_REACHED_END ...


def _lv_index_range(first_index, n):
    if not 0 <= int(first_index) <= 2 ** 32 - n:
        raise ValueError('simulation indices first_index .. first_index + batch - 1 must lie in [0, 2^32)')
    return int(first_index)


def lotka_volterra_draws(n, n_events, seed=0, stream=0, first_index=0, ctx=None):
    """(E, U), each (n, n_events): the unit exponentials and uniforms the drawn form of lotka_volterra_summaries uses for
    events 1 .. n_events of simulations first_index .. first_index + n - 1 -- Philox counter (i << 32) | k of (seed,
    stream).  Handing them back as draws=(E, U) reproduces the drawn form bit for bit."""
    n, n_events = int(n), int(n_events)
    if n < 1 or not 1 <= n_events <= LV_MAX_EVENTS:
        raise ValueError('need n >= 1 and 1 <= n_events <= 2^30')
    first_index = _lv_index_range(first_index, n)
    E, U = np.empty((n, n_events)), np.empty((n, n_events))
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_lv_draws", C.c_uint64(int(seed)), C.c_uint64(int(stream)), first_index, n, n_events, _lib.ptr(E),
             _lib.ptr(U))
    return E, U


def lotka_volterra_summaries(r1, r2, r3, prey_init=50, predator_init=100, sigma=None, n_obs=16, time_end=30.,
                             max_events=1 << 20, draws=None, noise=None, seed=0, stream=0, observed=None,
                             return_series=False, return_status=False, first_index=0, ctx=None):
    """The stochastic Lotka-Volterra example (elfi/examples/lotka_volterra.py) as ONE device operation: Gillespie's direct
    method for prey and predators with hazards r1 x, r2 x y, r3 y from floor(prey_init), floor(predator_init) up to
    time_end, the n_obs observations at np.linspace(0, time_end, n_obs) (linear interpolation between the bracketing
    events, plus sigma z when sigma is given, truncated as the reference's int32 array does) and the nine summaries
    LV_NAMES.  include/elfihip.h (elfihip_lv_summaries) states every operation.

    r1, r2, r3, prey_init, predator_init, sigma: (batch,) or scalars.  draws: (E, U), each (batch, n_events) -- unit
    exponentials and uniforms in [0, 1), column k - 1 for event k; they bound the events (max_events is then n_events).
    draws=None draws on the device: event k of simulation i reads Philox counter ((first_index + i) << 32) | k of (seed,
    stream), so a simulation does not depend on the batch it runs in.  noise: (batch, 2 (n_obs - 1)) standard normals, prey
    before predator for each observation (needs sigma); noise=None with sigma draws them from (seed, stream + 1).
    A simulation that has not reached time_end after max_events events is cut off: its remaining observations, its
    summaries and its distance are NaN (status 2; the reference has no bound and runs on).  Invalid parameters (a rate or
    sigma NaN, negative or infinite; an initial stock NaN, negative or >= 2^31) give a NaN row (status 3).
    observed: the 9 observed summaries; with them the euclidean distance is returned too.
    Returns S (batch, 9) [, series (batch, n_obs, 2)] [, status (batch,) int32, events (batch,) int64, final times
    (batch,)] [, d (batch,)] -- the bare array when nothing else is asked for."""
    n_obs, max_events = int(n_obs), int(max_events)
    if not 3 <= n_obs <= SERIES_MAX_OBS:
        raise ValueError('n_obs must be in [3, %d]' % SERIES_MAX_OBS)
    time_end = float(time_end)
    if not (np.isfinite(time_end) and time_end > 0):
        raise ValueError('time_end must be finite and positive')
    E = U = None
    if draws is not None:
        E, U = (np.asarray(a) for a in draws)
        if E.ndim != 2 or E.shape != U.shape or E.shape[1] < 1:
            raise ValueError('draws must be (E, U), each (batch, n_events)')
        max_events = E.shape[1]
    if not 1 <= max_events <= LV_MAX_EVENTS:
        raise ValueError('max_events must be in [1, 2^30]')
    if noise is not None:
        if sigma is None:
            raise ValueError('noise needs sigma')
        noise = np.asarray(noise)
        if noise.ndim != 2 or noise.shape[1] != 2 * (n_obs - 1):
            raise ValueError('noise must be (batch, 2 (n_obs - 1)) = (batch, %d)' % (2 * (n_obs - 1)))
    params = (r1, r2, r3, prey_init, predator_init) + (() if sigma is None else (sigma,))
    n = E.shape[0] if E is not None else noise.shape[0] if noise is not None else _batch_of(*params)
    if n < 1:
        raise ValueError('need at least one simulation')
    if noise is not None and noise.shape[0] != n:
        raise ValueError('noise must hold one row per simulation (%d)' % n)
    first_index = _lv_index_range(first_index, n)
    params = _params(n, *params)
    obs = None
    if observed is not None:
        obs = np.ascontiguousarray(np.asarray(observed, dtype=np.float64).reshape(-1))
        if obs.shape[0] != len(LV_NAMES):
            raise ValueError('observed must hold the %d observed summaries' % len(LV_NAMES))
    if E is not None:
        E, U = np.ascontiguousarray(E, dtype=np.float64), np.ascontiguousarray(U, dtype=np.float64)
    if noise is not None:
        noise = np.ascontiguousarray(noise, dtype=np.float64)
    S = np.empty((n, len(LV_NAMES)))
    Y = np.empty((n, n_obs, 2)) if return_series else None
    status = np.empty(n, dtype=np.int32) if return_status else None
    events = np.empty(n, dtype=np.int64) if return_status else None
    T = np.empty(n) if return_status else None
    D = np.empty(n) if obs is not None else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_lv_summaries", _lib.ptr(E), _lib.ptr(U), _lib.ptr(noise), C.c_uint64(int(seed)), C.c_uint64(int(stream)),
             first_index, n, n_obs, C.c_double(time_end), max_events, *[_lib.ptr(a) for a in params],
             *(() if sigma is not None else (None,)), _lib.ptr(obs), _lib.ptr(Y), _lib.ptr(T), _lib.ptr(status),
             _lib.ptr(events), _lib.ptr(S), _lib.ptr(D))
    out = tuple(a for a in (S, Y, status, events, T, D) if a is not None)
    return out if len(out) > 1 else S


# ---- the day-care-centre transmission example model (csrc/daycare.hip) ------------------------------------------------
DAYCARE_NAMES = ('Shannon', 'n_strains', 'prevalence', 'multi')
DAYCARE_MAX_EVENTS = 1 << 21                              # include/elfihip.h: ELFIHIP_DAYCARE_MAX_EVENTS
DAYCARE_MAX_DCC = 1024                                    # ELFIHIP_DAYCARE_MAX_DCC
DAYCARE_STATUS = ('reached_end', 'out_of_events', 'invalid')     # ELFIHIP_DAYCARE_REACHED_END ...


def _daycare_shape(n_dcc, n_ind=2, n_strains=1, n_obs=1):
    n_dcc, n_ind, n_strains, n_obs = int(n_dcc), int(n_ind), int(n_strains), int(n_obs)
    if not 1 <= n_dcc <= DAYCARE_MAX_DCC:
        raise ValueError('n_dcc must be in [1, %d]' % DAYCARE_MAX_DCC)
    if not 2 <= n_ind <= 64:
        raise ValueError('n_ind must be in [2, 64]')
    if not 1 <= n_strains <= 64:
        raise ValueError('n_strains must be in [1, 64]')
    if not 1 <= n_obs <= n_ind:
        raise ValueError('n_obs must be in [1, n_ind]')
    return n_dcc, n_ind, n_strains, n_obs


def daycare_draws(n, n_dcc, n_events, seed=0, stream=0, first_index=0, ctx=None):
    """(E, U), each (n, n_dcc, n_events): the unit exponentials and uniforms the drawn form of daycare_summaries uses for
    events 1 .. n_events of the centres of simulations first_index .. first_index + n - 1 -- Philox counter words ((centre <<
    22) | event, simulation) of (seed, stream).  Handing them back as draws=(E, U) reproduces the drawn form bit for bit."""
    n, n_events = int(n), int(n_events)
    n_dcc = _daycare_shape(n_dcc)[0]
    if n < 1 or not 1 <= n_events <= DAYCARE_MAX_EVENTS:
        raise ValueError('need n >= 1 and 1 <= n_events <= 2^21')
    first_index = _lv_index_range(first_index, n)
    E, U = np.empty((n, n_dcc, n_events)), np.empty((n, n_dcc, n_events))
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_daycare_draws", C.c_uint64(int(seed)), C.c_uint64(int(stream)), first_index, n, n_dcc, n_events,
             _lib.ptr(E), _lib.ptr(U))
    return E, U


def _daycare_observed(observed, k, m):
    obs = np.ascontiguousarray(np.asarray([np.asarray(o, dtype=np.float64).reshape(-1) for o in observed]
                                          if isinstance(observed, (list, tuple)) else observed, dtype=np.float64))
    if obs.size != k * m:
        raise ValueError('observed must hold %d summaries of %d columns' % (k, m))
    if not np.all(np.isfinite(obs)):
        raise ValueError('observed summaries must be finite')
    return obs.reshape(k, m)


def daycare_distance(*summaries, observed, ctx=None):
    """The day-care example's distance (elfi/examples/daycare.py: distance) on the device, usable as an elfi.Discrepancy
    operation: k summaries of shape (batch, m) and their k observed rows (1, m); every row divided by the observed row's
    maximum (1 where that is 0) and sorted, the L1 distance to the sorted observed row, summed over the summaries and divided
    by k m.  One array (batch, k, m) in place of the k summaries works too.  Returns (batch,); a NaN summary gives NaN."""
    if len(summaries) == 1 and np.ndim(summaries[0]) == 3:
        X = np.ascontiguousarray(summaries[0], dtype=np.float64)
    else:
        X = np.ascontiguousarray(np.stack([np.atleast_2d(np.asarray(s, dtype=np.float64)) for s in summaries], axis=1))
    if X.ndim != 3 or X.shape[0] < 1:
        raise ValueError('summaries must be k arrays of shape (batch, m)')
    n, k, m = X.shape
    if not (1 <= k <= 16 and 1 <= m <= DAYCARE_MAX_DCC and k * m <= 4096):
        raise ValueError('1 to 16 summaries of 1 to %d columns, at most 4096 values' % DAYCARE_MAX_DCC)
    obs = _daycare_observed(observed, k, m)
    D = np.empty(n)
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_daycare_distance", _lib.ptr(X), n, k, m, _lib.ptr(obs), _lib.ptr(D))
    return D


def daycare_summaries(t1, t2, t3, n_dcc=29, n_ind=53, n_strains=33, freq_strains_commun=None, n_obs=36, time_end=10.,
                      max_events=1 << 16, draws=None, seed=0, stream=0, observed=None, return_state=False, return_status=False,
                      first_index=0, ctx=None):
    """The day-care-centre transmission example (elfi/examples/daycare.py) as ONE device operation: Gillespie's direct method
    for the carriage of n_strains strains by the n_ind individuals of each of n_dcc centres up to time_end, and the four
    summaries DAYCARE_NAMES over the first n_obs individuals of every centre.  include/elfihip.h (elfihip_daycare_summaries)
    states every operation.

    t1, t2, t3: (batch,) or scalars.  Every centre stops at its own first event at or past time_end, so a simulation does not
    depend on the batch it runs in (the reference's lock-step does; it is reproduced exactly per centre).  draws: (E, U), each
    (batch, n_dcc, n_events) -- unit exponentials and uniforms in [0, 1), column k - 1 for event k; they bound the events
    (max_events is then n_events).  draws=None draws on the device from (seed, stream, first_index + simulation, centre,
    event).  A centre that has not reached time_end after max_events events has NaN summaries (status 1) and its simulation a
    NaN distance; t1, t2 or t3 NaN, negative or infinite gives NaN everywhere (status 2).
    observed: the (4, n_dcc) observed summaries; with them the example's distance is returned too.
    Returns S (batch, 4, n_dcc) [, state (batch, n_dcc, n_obs, n_strains) bool] [, status (batch, n_dcc) int32, events (batch,
    n_dcc) int64, final times (batch, n_dcc)] [, d (batch,)] -- the bare array when nothing else is asked for."""
    n_dcc, n_ind, n_strains, n_obs = _daycare_shape(n_dcc, n_ind, n_strains, n_obs)
    max_events = int(max_events)
    time_end = float(time_end)
    if not (np.isfinite(time_end) and time_end > 0):
        raise ValueError('time_end must be finite and positive')
    freq = None
    if freq_strains_commun is not None:
        freq = np.ascontiguousarray(np.asarray(freq_strains_commun, dtype=np.float64).reshape(-1))
        if freq.shape[0] != n_strains or not np.all(np.isfinite(freq) & (freq >= 0)):
            raise ValueError('freq_strains_commun must hold n_strains finite values that are not negative')
    E = U = None
    if draws is not None:
        E, U = (np.asarray(a) for a in draws)
        if E.ndim != 3 or E.shape != U.shape or E.shape[1] != n_dcc or E.shape[2] < 1:
            raise ValueError('draws must be (E, U), each (batch, n_dcc, n_events)')
        max_events = E.shape[2]
    if not 1 <= max_events <= DAYCARE_MAX_EVENTS:
        raise ValueError('max_events must be in [1, 2^21]')
    n = E.shape[0] if E is not None else _batch_of(t1, t2, t3)
    if n < 1:
        raise ValueError('need at least one simulation')
    first_index = _lv_index_range(first_index, n)
    params = _params(n, t1, t2, t3)
    obs = _daycare_observed(observed, len(DAYCARE_NAMES), n_dcc) if observed is not None else None
    if E is not None:
        E, U = np.ascontiguousarray(E, dtype=np.float64), np.ascontiguousarray(U, dtype=np.float64)
    S = np.empty((n, len(DAYCARE_NAMES), n_dcc))
    M = np.empty((n, n_dcc, n_obs), dtype=np.uint64) if return_state else None
    status = np.empty((n, n_dcc), dtype=np.int32) if return_status else None
    events = np.empty((n, n_dcc), dtype=np.int64) if return_status else None
    T = np.empty((n, n_dcc)) if return_status else None
    D = np.empty(n) if obs is not None else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_daycare_summaries", _lib.ptr(E), _lib.ptr(U), C.c_uint64(int(seed)), C.c_uint64(int(stream)), first_index,
             n, n_dcc, n_ind, n_strains, n_obs, C.c_double(time_end), max_events, *[_lib.ptr(a) for a in params], _lib.ptr(freq),
             _lib.ptr(obs), _lib.ptr(M), _lib.ptr(T), _lib.ptr(status), _lib.ptr(events), _lib.ptr(S), _lib.ptr(D))
    state = None
    if M is not None:
        state = ((M[..., None] >> np.arange(n_strains, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    out = tuple(a for a in (S, state, status, events, T, D) if a is not None)
    return out if len(out) > 1 else S


# ---- alpha-stable variates and Marchand's toad example model (csrc/stable.hpp, csrc/toad.hip) -----------------------
TOAD_MAX_CELLS = 8192                                     # include/elfihip.h: ELFIHIP_TOAD_MAX_CELLS
TOAD_MAX_LAGS = 8                                         # ELFIHIP_TOAD_MAX_LAGS
TOAD_MAX_QUANTILES = 64                                   # ELFIHIP_TOAD_MAX_QUANTILES
TOAD_LAGS = (1, 2, 4, 8)


def levy_stable(alpha, scale=1., seed=0, stream=0, angle=None, expo=None, ctx=None):
    """Symmetric (beta = 0) alpha-stable variates in the shape of `alpha`, S1 parameterisation, as float64: SciPy's
    levy_stable.rvs(alpha, beta=0, scale=scale) -- the Chambers-Mallows-Stuck transform of an angle TH and a standard
    exponential W in SciPy's order of operations (csrc/stable.hpp; include/elfihip.h states it).  Element e of the flattened
    array is a fixed function of alpha[e], scale[e] and Philox counter e of stream (seed, stream), so it does not depend on the
    batch, and a fused kernel that draws element e itself (the toad kernel does) gets the same number.  With `angle` and
    `expo` (both, in the shape of alpha) the transform is applied to those TH and W and nothing is drawn.  alpha == 1 is the
    Cauchy branch tan TH.  alpha outside (0, 2], NaN alpha or a negative or NaN scale gives NaN for that element."""
    alpha = np.asarray(alpha, dtype=np.float64)
    if (angle is None) != (expo is None):
        raise ValueError('angle and expo are given together or not at all')
    flat = np.ascontiguousarray(alpha.reshape(-1))
    n = flat.shape[0]
    scale = np.asarray(scale, dtype=np.float64)
    if scale.size not in (1, n):
        raise ValueError('scale must be a scalar or have the shape of alpha')
    scale = np.ascontiguousarray(np.broadcast_to(scale.reshape(-1), (n,)))
    TH = W = None
    if angle is not None:
        TH, W = [np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)) for a in (angle, expo)]
        if TH.shape[0] != n or W.shape[0] != n:
            raise ValueError('angle and expo must have the shape of alpha')
    out = np.empty(n)
    if n == 0:
        return out.reshape(alpha.shape)
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_stable", C.c_uint64(int(seed)), C.c_uint64(int(stream)), n, _lib.ptr(flat), _lib.ptr(scale), _lib.ptr(TH),
             _lib.ptr(W), _lib.ptr(out))
    return out.reshape(alpha.shape)


def _toad_shape(n_toads, n_days, lags, p, thd):
    n_toads, n_days = int(n_toads), int(n_days)
    if n_days < 2 or n_toads < 1 or n_days * n_toads > TOAD_MAX_CELLS:
        raise ValueError('need n_days >= 2, n_toads >= 1 and n_days * n_toads <= %d' % TOAD_MAX_CELLS)
    lags = np.ascontiguousarray(np.asarray(lags).reshape(-1))
    if not 1 <= lags.shape[0] <= TOAD_MAX_LAGS:
        raise ValueError('1 to %d lags' % TOAD_MAX_LAGS)
    if lags.dtype.kind not in 'iu' or not np.all((lags >= 1) & (lags <= n_days - 1)):
        raise ValueError('every lag must be an integer in [1, n_days - 1]')
    p = np.linspace(0, 1, 11) if p is None else np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1))
    if not 1 <= p.shape[0] <= TOAD_MAX_QUANTILES:
        raise ValueError('1 to %d quantiles' % TOAD_MAX_QUANTILES)
    if not (np.all((p >= 0) & (p <= 1)) and np.all(np.diff(p) > 0)):
        raise ValueError('quantiles must increase within [0, 1]')
    thd = float(thd)
    if thd != thd:
        raise ValueError('thd is NaN')
    return n_toads, n_days, lags.astype(np.int32), p, thd


def toad_summaries(alpha, gamma, p0, n_toads=66, n_days=63, lags=TOAD_LAGS, p=None, thd=10., draws=None, seed=0, stream=0,
                   first_index=0, return_series=False, return_steps=False, return_draws=False, ctx=None):
    """Marchand's toad movement example (elfi/examples/toad.py) as ONE device operation: the positions X[0] = 0, X[i] = X[r]
    for a toad that returns (probability p0) to the refuge of an earlier day r, X[i - 1] + dx otherwise, dx a symmetric
    alpha-stable step of scale gamma (elfi_amd.levy_stable's transform), and compute_summaries for every lag: the number of
    displacements |X[i + lag] - X[i]| below thd, np.nanmedian of the others and log(max(diff(np.nanquantile(others, p)),
    exp(-20))), NaN -> inf -- len(p) + 1 columns per lag (p: default np.linspace(0, 1, 11)), lag by lag, the reference's S1, S2,
    S4, S8 side by side.  include/elfihip.h (elfihip_toad_summaries) states every operation.

    alpha, gamma, p0: (batch,) or scalars.  draws: (U, TH, W, R), each (batch, n_days - 1, n_toads) -- per day the reference's
    uniform((n_toads, batch)), levy_stable's angle uniform * pi + (-pi / 2) and standard exponential, and choice(day, size),
    simulation first (tests/toad_ref.py: draws_from_state); R integers in [0, day).  draws=None draws on the device, a fixed
    function of (seed, stream, first_index + row, day, toad) that does not depend on the batch.
    An invalid parameter row (alpha outside (0, 2], gamma < 0, p0 outside [0, 1], NaN) has NaN summaries, positions and steps.
    Returns S (batch, (len(p) + 1) len(lags)) [, X (batch, n_days, n_toads) -- the reference's X is (n_days, n_toads, batch)]
    [, dx (batch, n_days - 1, n_toads), the step of every cell, used or not] [, (U, TH, W, R) the draws used] -- the bare array
    when nothing else is asked for."""
    n_toads, n_days, lags, p, thd = _toad_shape(n_toads, n_days, lags, p, thd)
    cells = (n_days - 1, n_toads)
    given = [None] * 4
    if draws is not None:
        given = [np.asarray(a) for a in draws]
        if len(given) != 4 or any(a.ndim != 3 or a.shape[1:] != cells or a.shape[0] != given[0].shape[0] for a in given):
            raise ValueError('draws must be (U, TH, W, R), each (batch, n_days - 1, n_toads) = (batch, %d, %d)' % cells)
        R = given[3]
        if R.dtype.kind not in 'iu' and not np.array_equal(R, np.floor(R)):
            raise ValueError('the refuge indices R must be integers')
        if R.size and not np.all((R >= 0) & (R < np.arange(1, n_days).reshape(1, -1, 1))):
            raise ValueError('the refuge index of day i must lie in [0, i)')
        given = [np.ascontiguousarray(a, dtype=np.float64) for a in given[:3]] + [np.ascontiguousarray(R, dtype=np.int32)]
    n = given[0].shape[0] if draws is not None else _batch_of(alpha, gamma, p0)
    if n < 1:
        raise ValueError('need at least one simulation')
    first_index = _lv_index_range(first_index, n)
    params = _params(n, alpha, gamma, p0)
    S = np.empty((n, (p.shape[0] + 1) * lags.shape[0]))
    X = np.empty((n, n_days, n_toads)) if return_series else None
    Dx = np.empty((n,) + cells) if return_steps else None
    echo = [np.empty((n,) + cells, dtype=t) if return_draws else None for t in (np.float64,) * 3 + (np.int32,)]
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_toad_summaries", *[_lib.ptr(a) for a in given], C.c_uint64(int(seed)), C.c_uint64(int(stream)), first_index,
             n, n_toads, n_days, lags.shape[0], _lib.ptr(lags), p.shape[0], _lib.ptr(p), C.c_double(thd),
             *[_lib.ptr(a) for a in params], _lib.ptr(S), _lib.ptr(X), _lib.ptr(Dx), *[_lib.ptr(a) for a in echo])
    out = tuple(a for a in (S, X, Dx, tuple(echo) if return_draws else None) if a is not None)
    return out if len(out) > 1 else S


# ---- general alpha-stable variates and the stochastic-volatility example (csrc/stable.hpp, csrc/sv.hip) ---------------
SV_MAX_OBS = 4096                                         # include/elfihip.h: ELFIHIP_SV_MAX_OBS
SV_Q_KURT = (.05, .25, .75, .95)
SV_Q_SKEW = (.05, .5, .95)


def levy_stable_general(alpha, beta, loc=0., scale=1., parameterization='S1', seed=0, stream=0, angle=None, expo=None, ctx=None):
    """Alpha-stable variates in the shape of `alpha`, as float64: SciPy 1.15's levy_stable.rvs(alpha, beta, loc, scale), per
    element and in SciPy's order of operations -- _rvs_Z1's branch (alpha == 1; beta == 0, elfi_amd.levy_stable's expression;
    otherwise) on an angle TH and a standard exponential W, Z scale + loc, rvs's shift at alpha == 1 and, for parameterization
    'S0', the shift to S0 (csrc/stable.hpp: stable_general; include/elfihip.h states every operation).  beta, loc, scale:
    scalars or in the shape of alpha.  Element e of the flattened array is a fixed function of its parameters and Philox
    counter e of stream (seed, stream): it does not depend on the batch, and at beta = 0, loc = 0, 'S1' it is
    elfi_amd.levy_stable's element e.  With `angle` and `expo` (both, in the shape of alpha) the transform is applied to those
    TH and W and nothing is drawn.
    The one difference from SciPy: alpha outside (0, 2], beta outside [-1, 1], a negative scale, or NaN in alpha, beta or scale
    gives NaN for that element alone, where SciPy raises for the whole call.  As in SciPy, scale == 0 at alpha == 1 is 0 log 0
    = NaN."""
    if parameterization not in ('S0', 'S1'):
        raise ValueError("parameterization must be 'S0' or 'S1'")
    alpha = np.asarray(alpha, dtype=np.float64)
    if (angle is None) != (expo is None):
        raise ValueError('angle and expo are given together or not at all')
    flat = np.ascontiguousarray(alpha.reshape(-1))
    n = flat.shape[0]
    others = []
    for name, a in (('beta', beta), ('loc', loc), ('scale', scale)):
        a = np.asarray(a, dtype=np.float64)
        if a.size not in (1, n):
            raise ValueError('%s must be a scalar or have the shape of alpha' % name)
        others.append(np.ascontiguousarray(np.broadcast_to(a.reshape(-1), (n,))))
    TH = W = None
    if angle is not None:
        TH, W = [np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)) for a in (angle, expo)]
        if TH.shape[0] != n or W.shape[0] != n:
            raise ValueError('angle and expo must have the shape of alpha')
    out = np.empty(n)
    if n == 0:
        return out.reshape(alpha.shape)
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_stable_general", C.c_uint64(int(seed)), C.c_uint64(int(stream)), n, int(parameterization == 'S0'),
             _lib.ptr(flat), *[_lib.ptr(a) for a in others], _lib.ptr(TH), _lib.ptr(W), _lib.ptr(out))
    return out.reshape(alpha.shape)


def _sv_quantiles(q_kurt, q_skew):
    qk, qs = [np.asarray(q, dtype=np.float64).reshape(-1) for q in (q_kurt, q_skew)]
    if qk.shape[0] != 4 or qs.shape[0] != 3:
        raise ValueError('q_kurt holds four probabilities and q_skew three')
    q = np.ascontiguousarray(np.concatenate([qk, qs]))
    if not np.all((q >= 0) & (q <= 1)):
        raise ValueError('quantile probabilities must lie in [0, 1]')
    return q


def sv_summaries(alpha, beta, kappa=1., eta=0., mu=0., phi=0.95, sigma=0.2, n_obs=50, x_0=None, draws=None, seed=0, stream=0,
                 first_index=0, q_kurt=SV_Q_KURT, q_skew=SV_Q_SKEW, return_series=True, return_logvol=False,
                 return_shocks=False, return_draws=False, ctx=None):
    """The alpha-stable stochastic-volatility example (elfi/examples/stochastic_volatility_model.py) as ONE device operation:
    the log-volatilities x[0] = z[0] sigma / sqrt(1 - min(phi^2, 0.99999)) + mu (with x_0: z[0] sigma + (mu + phi (x_0 - mu))),
    x[t] = z[t] sigma + (mu + phi (x[t - 1] - mu)); the shocks v[t], alpha-stable with skewness beta, location eta and scale
    kappa in the S0 parameterisation (elfi_amd.levy_stable_general's transform); the returns y[t] = exp(x[t] / 2) v[t]; and the
    reference's summaries kurt = (q95 - q05) / (q75 - q25) and skew = ((q95 - q50) - (q50 - q05)) / (q95 - q05) of np.quantile(y,
    q_kurt) and np.quantile(y, q_skew).  include/elfihip.h (elfihip_sv_summaries) states every operation.

    Every parameter is a scalar or (batch,); x_0 None is the stationary start.  draws: (Z, TH, W), each (batch, n_obs) -- the
    reference's n_obs calls of standard_normal(batch), then levy_stable's angle uniform((n_obs, batch)) * pi + (-pi / 2) and
    standard_exponential((n_obs, batch)), simulation first (tests/sv_ref.py: draws_from_state).  draws=None draws on the
    device, a fixed function of (seed, stream, first_index + row, t) that does not depend on the batch: TH and W from Philox
    counter ((first_index + row) << 32) | t of `stream` as levy_stable_general draws that counter, Z the first normal of that
    counter of `stream + 1`.  1 <= n_obs <= 4096.
    An invalid parameter row (alpha outside (0, 2], beta outside [-1, 1], kappa < 0, sigma < 0, or a NaN parameter) is NaN
    throughout, for that row alone -- SciPy raises for the whole batch.  A NaN in y makes both summaries NaN.
    Returns S (batch, 2) = [kurt, skew] [, y (batch, n_obs)] [, x (batch, n_obs)] [, v (batch, n_obs)] [, (Z, TH, W) the draws
    used] -- the bare array when nothing else is asked for."""
    n_obs = int(n_obs)
    if not 1 <= n_obs <= SV_MAX_OBS:
        raise ValueError('need 1 <= n_obs <= %d' % SV_MAX_OBS)
    q = _sv_quantiles(q_kurt, q_skew)
    given = [None] * 3
    if draws is not None:
        given = [np.asarray(a) for a in draws]
        if len(given) != 3 or any(a.ndim != 2 or a.shape != (given[0].shape[0], n_obs) for a in given):
            raise ValueError('draws must be (Z, TH, W), each (batch, n_obs) = (batch, %d)' % n_obs)
        given = [np.ascontiguousarray(a, dtype=np.float64) for a in given]
    ps = [alpha, beta, kappa, eta, mu, phi, sigma] + ([x_0] if x_0 is not None else [])
    n = given[0].shape[0] if draws is not None else _batch_of(*ps)
    if n < 1:
        raise ValueError('need at least one simulation')
    first_index = _lv_index_range(first_index, n)
    params = _params(n, *ps)
    if x_0 is None:
        params.append(None)
    S = np.empty((n, 2))
    Y, X, V = [np.empty((n, n_obs)) if flag else None for flag in (return_series, return_logvol, return_shocks)]
    echo = [np.empty((n, n_obs)) if return_draws else None for _ in range(3)]
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_sv_summaries", *[_lib.ptr(a) for a in given], C.c_uint64(int(seed)), C.c_uint64(int(stream)), first_index,
             n, n_obs, _lib.ptr(q), *[_lib.ptr(a) for a in params], _lib.ptr(S), _lib.ptr(Y), _lib.ptr(X), _lib.ptr(V),
             *[_lib.ptr(a) for a in echo])
    out = tuple(a for a in (S, Y, X, V, tuple(echo) if return_draws else None) if a is not None)
    return out if len(out) > 1 else S


# ---- the scratch-assay example model (csrc/scratch_assay.hip) ------------------------------------------------------------
ASSAY_MAX_CELLS = 1024                                    # include/elfihip.h: ELFIHIP_ASSAY_MAX_CELLS
ASSAY_MAX_ITER = 1 << 21                                  # ELFIHIP_ASSAY_MAX_ITER
ASSAY_STATUS = ('ok', 'bad_draw')                         # ELFIHIP_ASSAY_OK, ELFIHIP_ASSAY_BAD_DRAW


def scratch_assay_shape(obs_period=12, obs_interval=1 / 12, tau=1 / 24):
    """(n_iter, obs_every, n_obs) as elfi/examples/scratch_assay.py:73-75 computes them: int(obs_period / tau), int(obs_interval
    / tau), int(n_iter / obs_every).  The device takes only these integers."""
    with np.errstate(all='ignore'):
        ratio, every = np.float64(obs_period) / np.float64(tau), np.float64(obs_interval) / np.float64(tau)
    if not (np.isfinite(ratio) and np.isfinite(every) and 1 <= ratio <= ASSAY_MAX_ITER and every >= 1):
        raise ValueError('need 1 <= int(obs_period / tau) <= 2^21 iterations and int(obs_interval / tau) >= 1')
    n_iter, obs_every = int(ratio), int(every)
    if obs_every > n_iter:
        raise ValueError('no observation: int(obs_interval / tau) = %d exceeds the %d iterations' % (obs_every, n_iter))
    return n_iter, obs_every, int(n_iter / obs_every)


def _assay_grid(init_arr):
    init = np.asarray(init_arr)
    if init.ndim != 2 or not 1 <= init.size <= ASSAY_MAX_CELLS:
        raise ValueError('init_arr must be a grid (nrows, ncols) of 1 to %d cells' % ASSAY_MAX_CELLS)
    if not np.all((init == 0) | (init == 1)):
        raise ValueError('init_arr must hold zeros and ones')
    return np.ascontiguousarray(init, dtype=np.uint8)


def scratch_assay_draws(num_cells, n_cells, seed=0, stream=0, first_index=0, ctx=None):
    """(C, P, M), each (n, n_iter, 2, n_cells) -- int32 candidates, float64 uniforms, uint8 directions: what the drawn form of
    scratch_assay_summaries uses in phase f of iteration t of simulations first_index .. first_index + n - 1 when that phase
    has num_cells[i, t, f] slots (zero past them): one Philox call per slot, counter words (((2 t + f) << 10) | slot,
    simulation) of (seed, stream).  Handing them back as draws=(C, P, M) reproduces the drawn form bit for bit."""
    num = np.ascontiguousarray(num_cells, dtype=np.int32)
    n_cells = int(n_cells)
    if num.ndim != 3 or num.shape[2] != 2 or num.shape[0] < 1 or not 1 <= num.shape[1] <= ASSAY_MAX_ITER:
        raise ValueError('num_cells must be (n, n_iter, 2) with n >= 1 and 1 <= n_iter <= 2^21')
    if not 1 <= n_cells <= ASSAY_MAX_CELLS or num.min() < 0 or num.max() > n_cells:
        raise ValueError('need 1 <= n_cells <= %d and 0 <= num_cells <= n_cells' % ASSAY_MAX_CELLS)
    n, n_iter = num.shape[:2]
    first_index = _lv_index_range(first_index, n)
    Cd, P, M = (np.empty((n, n_iter, 2, n_cells), dtype=t) for t in (np.int32, np.float64, np.uint8))
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_assay_draws", C.c_uint64(int(seed)), C.c_uint64(int(stream)), first_index, n, n_iter, n_cells, _lib.ptr(num),
             _lib.ptr(Cd), _lib.ptr(P), _lib.ptr(M))
    return Cd, P, M


def scratch_assay_summaries(pm, pp, init_arr, obs_period=12, obs_interval=1 / 12, tau=1 / 24, seed=0, stream=0, first_index=0,
                            draws=None, return_frames=False, return_events=False, ctx=None):
    """The scratch-assay example (elfi/examples/scratch_assay.py: cell_sim and cell_summaries) as ONE device operation: the
    random walk with proliferation of the cells of the binary grid init_arr (nrows, ncols), at most 1024 cells, shared by the
    batch, over int(obs_period / tau) iterations, and the summaries of Price et al. (2018) -- the number of cells that differ
    between consecutive frames, a frame every int(obs_interval / tau) iterations, then the last frame's cell count.
    include/elfihip.h (elfihip_assay_summaries) states every operation.

    pm, pp: (batch,) or scalars, compared as they come (NaN selects nothing; no value is invalid).  draws: (C, P, M), each
    (batch, n_iter, 2, nrows ncols) -- int32 candidates, float64 uniforms, uint8 directions per slot of the motility and the
    proliferation phase of every iteration; entries past the current cell count are not read, and a candidate outside [0,
    cell count) or a direction above 3 that IS read ends that simulation with status 1, NaN summaries, empty frames.
    draws=None draws on the device from (seed, stream, first_index + simulation, iteration, phase, slot), so a simulation does
    not depend on the batch it runs in.  The reference's RandomState stream is not reproduced: its choice() rejects, the
    device's candidate is the high half of word x cell count (bias below 2.4e-7).
    Returns S (batch, n_obs + 1) [, frames (batch, nrows, ncols, n_obs + 1) uint8, the reference's layout] [, status (batch,)
    int32, events (batch, 2) int64: motility and proliferation events executed] -- the bare array when nothing else is asked
    for."""
    init = _assay_grid(init_arr)
    nrows, ncols = init.shape
    n_iter, obs_every, n_obs = scratch_assay_shape(obs_period, obs_interval, tau)
    Cd = P = M = None
    if draws is not None:
        Cd, P, M = (np.asarray(a) for a in draws)
        want = (n_iter, 2, nrows * ncols)
        if Cd.ndim != 4 or Cd.shape[1:] != want or P.shape != Cd.shape or M.shape != Cd.shape:
            raise ValueError('draws must be (C, P, M), each (batch, n_iter, 2, cells) = (batch, %d, 2, %d)' % (n_iter, want[2]))
        Cd, P, M = (np.ascontiguousarray(a, dtype=t) for a, t in ((Cd, np.int32), (P, np.float64), (M, np.uint8)))
    n = Cd.shape[0] if Cd is not None else _batch_of(pm, pp)
    if n < 1:
        raise ValueError('need at least one simulation')
    first_index = _lv_index_range(first_index, n)
    pm, pp = _params(n, pm, pp)
    S = np.empty((n, n_obs + 1))
    frames = np.empty((n, n_obs + 1, ASSAY_MAX_CELLS // 32), dtype=np.uint32) if return_frames else None
    status = np.empty(n, dtype=np.int32) if return_events else None
    events = np.empty((n, 2), dtype=np.int64) if return_events else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_assay_summaries", _lib.ptr(Cd), _lib.ptr(P), _lib.ptr(M), C.c_uint64(int(seed)), C.c_uint64(int(stream)),
             first_index, n, nrows, ncols, n_iter, obs_every, _lib.ptr(init), _lib.ptr(pm), _lib.ptr(pp), _lib.ptr(S),
             _lib.ptr(status), _lib.ptr(events), _lib.ptr(frames))
    if frames is not None:
        bits = np.unpackbits(frames.view(np.uint8), axis=2, bitorder='little')[:, :, :nrows * ncols]
        frames = np.ascontiguousarray(bits.reshape(n, n_obs + 1, nrows, ncols).transpose(0, 2, 3, 1))
    out = tuple(a for a in (S, frames, status, events) if a is not None)
    return out if len(out) > 1 else S


# ---- the birth-death-mutation example model (csrc/bdm.hip) ----------------------------------------------------------------
BDM_MAX_N = 4096                                          # include/elfihip.h: ELFIHIP_BDM_MAX_N
BDM_MAX_EVENTS = 1 << 30                                  # ELFIHIP_BDM_MAX_EVENTS
BDM_STATUS = ('reached_n', 'extinct', 'out_of_events', 'invalid')     # ELFIHIP_BDM_REACHED_N ...


def bdm_draws(n, n_events, seed=0, stream=0, first_index=0, ctx=None):
    """U (n, 2 n_events): the uniforms the drawn form of bdm_clusters uses for events 1 .. n_events of simulations first_index
    .. first_index + n - 1 -- column 2 (k - 1) chooses the event, the next one the cluster; Philox counter (i << 32) | k of
    (seed, stream).  Handing them back as draws=U reproduces the drawn form bit for bit."""
    n, n_events = int(n), int(n_events)
    if n < 1 or not 1 <= n_events <= BDM_MAX_EVENTS:
        raise ValueError('need n >= 1 and 1 <= n_events <= 2^30')
    first_index = _lv_index_range(first_index, n)
    U = np.empty((n, 2 * n_events))
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_bdm_draws", C.c_uint64(int(seed)), C.c_uint64(int(stream)), first_index, n, n_events, _lib.ptr(U))
    return U


def bdm_clusters(alpha, delta=0., tau=0.198, N=20, mode=1, max_events=1 << 16, draws=None, seed=0, stream=0, first_index=0,
                 observed=None, t2_n=None, return_summaries=False, return_status=False, ctx=None):
    """The birth-death-mutation example (elfi/examples/bdm.py and its cpp/bdm.cpp) as ONE device operation: the jump chain
    of births (rate alpha), deaths (delta) and mutations (tau) from one individual until the population reaches N, its
    cluster sizes and the summaries T1 and T2.  include/elfihip.h (elfihip_bdm_clusters) states every operation.  No
    executable, no files; the parameters are NOT rounded to 4 decimals as the reference's text file does.

    alpha, delta, tau: (batch,) or scalars.  N: 1 .. 4096, the length of the cluster vector.  mode 1 (the example's): stop
    just before the population would exceed N (Stadler 2011); mode 0: stop on reaching N (Tanaka et al. 2006).  draws: U
    (batch, 2 n_events) uniforms in [0, 1), columns 2 (k - 1) and 2 (k - 1) + 1 for event k; they bound the events (max_events
    is then n_events); one that is NaN or outside [0, 1) ends its own simulation with status 3.  draws=None draws on the
    device: event k of simulation i reads Philox counter ((first_index + i) << 32) | k of (seed, stream), so a simulation
    does not depend on the batch it runs in.  A simulation still running after max_events events is cut off: clusters as
    they stand, NaN summaries (status 2; the reference has no bound, and never returns with alpha = delta = 0).  An extinct
    population (status 1) has clusters 0, T1 NaN and T2 1, as NumPy gives.  Invalid rates (NaN, negative, infinite, or all
    zero) give zero clusters and NaN summaries (status 3).
    t2_n: the divisor of T2 (None: N, the reference's default of 20 at the example's N).  observed: the observed T1; with it
    the example's distance |T1 - observed| is returned too.
    Returns clusters (batch, N) int32 [, T (batch, 2): T1, T2] [, status (batch,) int32, events (batch,) int64] [, d
    (batch,)] -- the bare array when nothing else is asked for."""
    N, mode, max_events = int(N), int(mode), int(max_events)
    if not 1 <= N <= BDM_MAX_N:
        raise ValueError('N must be in [1, %d]' % BDM_MAX_N)
    if mode not in (0, 1):
        raise ValueError('mode must be 0 (stop on reaching N) or 1 (stop before exceeding N)')
    U = None
    if draws is not None:
        U = np.asarray(draws)
        if U.ndim != 2 or U.shape[1] < 2 or U.shape[1] % 2:
            raise ValueError('draws must be (batch, 2 n_events)')
        max_events = U.shape[1] // 2
    if not 1 <= max_events <= BDM_MAX_EVENTS:
        raise ValueError('max_events must be in [1, 2^30]')
    n = U.shape[0] if U is not None else _batch_of(alpha, delta, tau)
    if n < 1:
        raise ValueError('need at least one simulation')
    first_index = _lv_index_range(first_index, n)
    alpha, delta, tau = _params(n, alpha, delta, tau)
    t2_n = float(N if t2_n is None else t2_n)
    obs = None
    if observed is not None:
        obs = np.ascontiguousarray(np.asarray(observed, dtype=np.float64).reshape(-1))
        if obs.shape[0] != 1:
            raise ValueError('observed must hold the one observed summary T1')
    if U is not None:
        U = np.ascontiguousarray(U, dtype=np.float64)
    Cl = np.empty((n, N), dtype=np.int32)
    T = np.empty((n, 2)) if return_summaries else None
    status = np.empty(n, dtype=np.int32) if return_status else None
    events = np.empty(n, dtype=np.int64) if return_status else None
    D = np.empty(n) if obs is not None else None
    ctx = ctx or _lib.default_context()
    ctx.call("elfihip_bdm_clusters", _lib.ptr(U), C.c_uint64(int(seed)), C.c_uint64(int(stream)), first_index, n, N, mode,
             max_events, _lib.ptr(alpha), _lib.ptr(delta), _lib.ptr(tau), C.c_double(t2_n), _lib.ptr(obs), _lib.ptr(Cl),
             _lib.ptr(status), _lib.ptr(events), _lib.ptr(T), _lib.ptr(D))
    out = tuple(a for a in (Cl, T, status, events, D) if a is not None)
    return out if len(out) > 1 else Cl
