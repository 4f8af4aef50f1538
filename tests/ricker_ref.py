"""NumPy statement of the Ricker example model the device runs (csrc/series.hip: ricker_kernel) and of the library's
counter-based Poisson sampler (csrc/poisson.hpp).

The model functions are written from the model's definition, draws handed in, in the operation order the device keeps;
they are pinned bit for bit to recorded runs of ELFI's own example (tests/golden/ricker.npz, tests/test_ricker.py).  The
sampler is the rule of include/elfihip.h (elfihip_poisson) on the uniforms of tests/philox_ref.py; next to every draw it
says whether the draw is BOUNDARY-SENSITIVE: decided so closely that an exp, log or lgamma that differs from the host's in
the last places may decide it the other way.  The device is held to this statement exactly outside that mask
(tests/test_ricker_gpu.py).
"""
import numpy as np

import philox_ref as P

MAX_K, MAX_ATTEMPTS = 128, 64          # include/elfihip.h: ELFIHIP_POISSON_MAX_K, ELFIHIP_POISSON_MAX_ATTEMPTS
LAM_MAX = 2.0 ** 53
EPS = np.finfo(np.float64).eps


def uniform53_pair(seed, stream, idx):
    """(u1, u2) of Philox counter `idx` of stream (seed, stream): words 0, 1 and words 2, 3 as 53-bit uniforms in [0, 1)."""
    u64 = np.uint64
    idx = np.asarray(idx, dtype=u64)
    lo, s32 = u64(0xffffffff), u64(32)
    seed, stream = u64(int(seed) & (2 ** 64 - 1)), u64(int(stream) & (2 ** 64 - 1))
    r = P.philox4x32_10_vec((idx & lo, idx >> s32, stream & lo, stream >> s32), (seed & lo, seed >> s32))
    u1 = ((r[0] << u64(21)) | (r[1] >> u64(11))).astype(np.float64) * 2.0 ** -53
    u2 = ((r[2] << u64(21)) | (r[3] >> u64(11))).astype(np.float64) * 2.0 ** -53
    return u1, u2


def poisson_ref(lam, seed, stream, return_attempts=False):
    """(draws, sensitive [, attempts]) in the shape of `lam`: element e of the flattened array is poisson_draw(lam[e], seed,
    stream, e).  sensitive[e] is True when
      * |u1 - F_k| <= 2^-44 for a cumulative probability F_k the inversion visited,
      * the argument of the PTRS floor is within 8 ulp of an integer,
      * us is within 1e-12 of 0.07 or 0.013, or V within 1e-12 of vr (or of us, where that test is reached),
      * the two sides of the log test differ by at most 64 eps (lam + |k loglam| + lgamma(k + 1) + |lhs|)
    in any attempt made.  attempts: the number of uniform pairs read (0 for lam == 0 and invalid lam)."""
    from scipy.special import gammaln
    lam = np.asarray(lam, dtype=np.float64)
    shape = lam.shape
    lam = lam.reshape(-1)
    n = lam.shape[0]
    out = np.full(n, np.nan)
    sens = np.zeros(n, dtype=bool)
    attempts = np.zeros(n, dtype=np.int64)
    with np.errstate(all='ignore'):
        valid = (lam >= 0) & (lam <= LAM_MAX)
        out[valid & (lam == 0)] = 0.0
        # inversion
        ii = np.flatnonzero(valid & (lam > 0) & (lam < 10.0))
        if ii.size:
            l = lam[ii]
            u1, _ = uniform53_pair(seed, stream, ii)
            attempts[ii] = 1
            p = np.exp(-l)
            F = p.copy()
            k = np.zeros(ii.size)
            s = np.abs(u1 - F) <= 2.0 ** -44
            act = u1 > F
            for _ in range(MAX_K):
                if not act.any():
                    break
                k = np.where(act, k + 1, k)
                pn = p * (l / np.where(act, k, 1.0))
                p = np.where(act, pn, p)
                F = np.where(act, F + p, F)
                s |= act & (np.abs(u1 - F) <= 2.0 ** -44)
                act = act & (u1 > F)
            out[ii] = k
            sens[ii] = s
        # PTRS
        ii = np.flatnonzero(valid & (lam >= 10.0))
        if ii.size:
            out[ii] = np.floor(lam[ii])          # what remains if every attempt rejects
        for j in range(MAX_ATTEMPTS):
            if not ii.size:
                break
            l = lam[ii]
            slam, loglam = np.sqrt(l), np.log(l)
            b = 0.931 + 2.53 * slam
            a = -0.059 + 0.02483 * b
            invalpha = 1.1239 + 1.1328 / (b - 3.4)
            vr = 0.9277 - 3.6224 / (b - 2.0)
            u1, u2 = uniform53_pair(seed, int(stream) + j, ii)
            attempts[ii] += 1
            U, V = u1 - 0.5, u2
            us = 0.5 - np.abs(U)
            x = (((2.0 * a) / us + b) * U + l) + 0.43
            k = np.floor(x)
            s = np.isfinite(x) & (np.abs(x - np.round(x)) <= 8 * np.spacing(np.abs(x)))
            s |= (np.abs(us - 0.07) <= 1e-12) | (np.abs(us - 0.013) <= 1e-12) | (np.abs(V - vr) <= 1e-12)
            fast = (us >= 0.07) & (V <= vr)
            s |= ~fast & (us < 0.013 + 1e-12) & (np.abs(V - us) <= 1e-12)
            rej = ~fast & ((k < 0) | ((us < 0.013) & (V > us)))
            slow = ~fast & ~rej
            lhs = (np.log(V) + np.log(invalpha)) - np.log(a / (us * us) + b)
            kk = np.where(slow, k, 0.0)
            lg = gammaln(kk + 1.0)
            rhs = (-l + kk * loglam) - lg
            s |= slow & (np.abs(lhs - rhs) <= 64 * EPS * (l + np.abs(kk * loglam) + lg + np.abs(lhs)))
            acc = fast | (slow & (lhs <= rhs))
            sens[ii] |= s
            out[ii[acc]] = k[acc]
            ii = ii[~acc]
    res = (out.reshape(shape), sens.reshape(shape))
    return res + (attempts.reshape(shape),) if return_attempts else res


# ---- the model ------------------------------------------------------------------------------------------------------
def _col(t, batch):
    return np.broadcast_to(np.asarray(t, dtype=np.float64).reshape(-1), (batch,))


def ricker_step(log_rate, std, s, z):
    """One step of the stochastic recurrence in the reference's operation order: s exp((log_rate - s) + std z)."""
    with np.errstate(all='ignore'):
        return s * np.exp(log_rate - s + std * z)


def ricker_stock(log_rate, std, Z, stock_init=1.):
    """Latent stock (batch, n_obs): s_0 = stock_init, s_i = s_{i-1} exp((log_rate - s_{i-1}) + std Z[:, i - 1])."""
    Z = np.asarray(Z, dtype=np.float64)
    batch, n_obs = Z.shape
    log_rate, std = _col(log_rate, batch), _col(std, batch)
    s = np.full(batch, float(stock_init))
    St = np.empty((batch, n_obs))
    for i in range(n_obs):
        s = ricker_step(log_rate, std, s, Z[:, i])
        St[:, i] = s
    return St


def ricker_series_deterministic(log_rate, stock_init=1., n_obs=50):
    """The deterministic model (batch, n_obs): y_0 = stock_init, y_i = y_{i-1} exp(log_rate - y_{i-1})."""
    log_rate = np.asarray(log_rate, dtype=np.float64).reshape(-1)
    Y = np.empty((log_rate.shape[0], n_obs))
    Y[:, 0] = stock_init
    with np.errstate(all='ignore'):
        for i in range(1, n_obs):
            Y[:, i] = Y[:, i - 1] * np.exp(log_rate - Y[:, i - 1])
    return Y


def stochastic_ricker_from_state(rs, log_rate, std, scale, stock_init=1., n_obs=50, batch=1):
    """(Z, St, Y), each (batch, n_obs): the reference's own interleaved calls -- randn(batch), then poisson(scale stock,
    batch), once per step -- on the RandomState `rs`."""
    Z, St, Y = [np.empty((batch, n_obs)) for _ in range(3)]
    s = stock_init
    for i in range(n_obs):
        Z[:, i] = rs.randn(batch)
        s = ricker_step(log_rate, std, s, Z[:, i])
        St[:, i] = s
        Y[:, i] = rs.poisson(scale * s, batch)
    return Z, St, Y


def ricker_summaries(Y):
    """(batch, 3) = Mean, Var, #0: np.mean, np.var (ddof 0) and the number of zeros along each row."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    with np.errstate(all='ignore'):
        return np.column_stack((np.mean(Y, axis=1), np.var(Y, axis=1), np.sum(Y == 0, axis=1).astype(np.float64)))


def chi_squared(S, obs):
    """The reference's chi_squared on the rows of S against the observed summaries: sum((S - obs)^2 / obs, axis=1)."""
    S = np.atleast_2d(np.asarray(S, dtype=np.float64))
    obs = np.asarray(obs, dtype=np.float64).reshape(1, -1)
    with np.errstate(all='ignore'):
        return np.sum((S - obs) ** 2. / obs, axis=1)
