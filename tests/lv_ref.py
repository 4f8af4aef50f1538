"""NumPy statement of the stochastic Lotka-Volterra model the device runs (csrc/gillespie.hip): Gillespie's direct method
for prey x and predators y with hazards r1 x, r2 x y, r3 y, observed at n_obs evenly spaced times by linear interpolation
between the two events that bracket each time, and the nine summaries of the example.

The simulator is written from the model's definition (include/elfihip.h: elfihip_lv_summaries), vectorised in lock-step
over the batch from given draws E (unit exponentials), U (uniforms in [0, 1)) and Z (standard normals), in the operation
order the device keeps; it is pinned bit for bit to recorded runs of ELFI's own example (tests/golden/lotka_volterra.npz,
tests/test_lotka_volterra.py).  draws() states the Philox layout of the drawn form, and simulate(return_mask=True) names
the observations that a last-bit difference in an event time (the device's log is not the host's) may move.
"""
import numpy as np

import philox_ref as P

EPS = np.finfo(np.float64).eps
NAMES = ('prey_mean', 'pred_mean', 'prey_log_var', 'pred_log_var', 'prey_autocorr_1', 'pred_autocorr_1',
         'prey_autocorr_2', 'pred_autocorr_2', 'crosscorr')
REACHED_END, EXTINCT, OUT_OF_EVENTS, INVALID = 0, 1, 2, 3
INT_LIMIT = 2.0 ** 31


def _col(t, batch):
    return np.array(np.broadcast_to(np.asarray(t, dtype=np.float64).reshape(-1), (batch,)))


def times_out(time_end, n_obs):
    """np.linspace(0, time_end, n_obs) spelled out: i * step, the last element time_end itself."""
    step = float(time_end) / (n_obs - 1)
    t = np.arange(0, n_obs) * step
    t[-1] = time_end
    return t


def store_int(v):
    """What an int32 slot keeps of v, as a double: truncated toward zero, -0 as +0; NaN where int32 cannot hold it."""
    with np.errstate(invalid='ignore'):
        out = np.trunc(v) + 0.0
        out[~(np.abs(v) < INT_LIMIT)] = np.nan
    return out


def simulate(r1, r2, r3, prey_init, predator_init, sigma, E, U, Z=None, n_obs=16, time_end=30., return_chain=False,
             return_mask=False):
    """(Y (n, n_obs, 2), t_final (n), status (n) int32, events (n) int64 [, chain] [, mask]) from given draws: column
    k - 1 of E and U feeds event k, max_events = E.shape[1]; Z (n, 2 (n_obs - 1)) with sigma, prey before predator.
    chain: the list of (x, y, t) after every event, rows frozen once finished, for comparing jump chains.
    mask (n, n_obs) bool: the observations that event times differing in their last bits (the device's log is not the
    host's) may change -- a bracketing event time within 64 eps t of the observation time (the observation may then
    belong to a neighbouring event, or the simulation stop an event later), or a noisy value within 64 eps |v| of a
    whole number (its truncation may differ; without noise a value is whole only where the time test already marks it).  A time forced to time_end by extinction is exact."""
    E, U = np.asarray(E, dtype=np.float64), np.asarray(U, dtype=np.float64)
    n, max_events = E.shape
    r1, r2, r3 = _col(r1, n), _col(r2, n), _col(r3, n)
    noisy = sigma is not None
    sg = _col(sigma, n) if noisy else np.zeros(n)
    tout = times_out(time_end, n_obs)
    with np.errstate(all='ignore'):
        x, y = np.floor(_col(prey_init, n)), np.floor(_col(predator_init, n))
        ok_rate = lambda r: np.isfinite(r) & (r >= 0)
        ok_init = lambda s: (s >= 0) & (s < INT_LIMIT)
        valid = ok_rate(r1) & ok_rate(r2) & ok_rate(r3) & ok_rate(sg) & ok_init(x) & ok_init(y)
        Y = np.full((n, n_obs, 2), np.nan)
        Y[:, 0, 0], Y[:, 0, 1] = x, y
        t = np.zeros(n)
        nxt = np.ones(n, dtype=np.int64)                # the next observation to emit
        events = np.zeros(n, dtype=np.int64)
        status = np.full(n, OUT_OF_EVENTS, dtype=np.int32)
        status[~valid] = INVALID
        live = valid.copy()
        chain = []
        mask = np.zeros((n, n_obs), dtype=bool)
        for k in range(1, max_events + 1):
            if not live.any():
                break
            e, u = E[:, k - 1], U[:, k - 1]
            h0 = r1 * x
            h1 = (r2 * x) * y
            h2 = r3 * y
            s = (h0 + h1) + h2
            inv = 1.0 / s
            t_new = t + inv * e
            p0 = h0 * inv
            p1 = h1 * inv
            c0, c1 = p0, p0 + p1
            reaction = (u >= c0).astype(np.int64) + (u >= c1)
            reaction[np.isinf(inv)] = 3
            x_new = x + np.array([1., -1., 0., 0.])[reaction]
            y_new = y + np.array([0., 1., -1., 0.])[reaction]
            forced = y_new == 0
            t_new = np.where(forced, time_end, t_new)
            while True:                                 # rows whose event passes their next observation time
                hit = live & (nxt < n_obs)
                to = tout[np.minimum(nxt, n_obs - 1)]
                hit &= t_new >= to
                if not hit.any():
                    break
                i, to = nxt[hit], to[hit]
                term = (to - t[hit]) / (t_new[hit] - t[hit])
                vx = (x_new[hit] - x[hit]) * term + x[hit]
                vy = (y_new[hit] - y[hit]) * term + y[hit]
                if noisy:
                    vx = vx + sg[hit] * Z[hit, 2 * (i - 1)]
                    vy = vy + sg[hit] * Z[hit, 2 * (i - 1) + 1]
                Y[hit, i, 0], Y[hit, i, 1] = store_int(vx), store_int(vy)
                if return_mask:
                    tol = 64 * EPS * to
                    near = (np.abs(t[hit] - to) <= tol) | (~forced[hit] & (np.abs(t_new[hit] - to) <= tol))
                    if noisy:
                        for v in (vx, vy):
                            near |= np.abs(v - np.round(v)) <= 64 * EPS * np.maximum(np.abs(v), 1.0)
                    mask[hit, i] = near
                nxt[hit] += 1
            x, y, t = np.where(live, x_new, x), np.where(live, y_new, y), np.where(live, t_new, t)
            events[live] = k
            done = live & (t >= time_end)
            status[done] = np.where(y[done] == 0, EXTINCT, REACHED_END)
            live &= ~done
            if return_chain:
                chain.append((x.copy(), y.copy(), t.copy()))
        Y[~valid] = np.nan
        t[~valid] = np.nan
    out = (Y, t, status, events)
    if return_chain:
        out += (chain,)
    if return_mask:
        out += (mask,)
    return out


def draws(seed, stream, n, n_events, first=0):
    """(E, U, A), each (n, n_events): event k of simulation i reads Philox counter ((first + i) << 32) | k of (seed,
    stream); E = -log((a + 1) 2^-53) with a the 53 bits of words 0, 1 (A, returned for the ulp comparison), U = the 53 bits
    of words 2, 3 times 2^-53."""
    u64 = np.uint64
    i = (np.arange(n, dtype=u64) + u64(first))[:, None]
    k = np.arange(1, n_events + 1, dtype=u64)[None, :]
    c0, c1 = np.broadcast_arrays(k, i)
    lo, s32 = u64(0xffffffff), u64(32)
    seed, stream = u64(int(seed) & (2 ** 64 - 1)), u64(int(stream) & (2 ** 64 - 1))
    zero = np.zeros_like(c0)
    r = P.philox4x32_10_vec((c0.copy(), c1.copy(), zero + (stream & lo), zero + (stream >> s32)), (seed & lo, seed >> s32))
    a = (r[0] << u64(21)) | (r[1] >> u64(11))
    b = (r[2] << u64(21)) | (r[3] >> u64(11))
    A = (a + u64(1)).astype(np.float64) * 2.0 ** -53
    return -np.log(A), b.astype(np.float64) * 2.0 ** -53, A


# ---- the nine summaries -------------------------------------------------------------------------------------------------
def _species(Y, species):
    return np.ascontiguousarray(np.asarray(Y, dtype=np.float64)[:, :, species])


def stock_mean(Y, species):
    return np.mean(_species(Y, species), axis=1)


def variance_plus_one(Y, species):
    """The argument of the log-variance's logarithm: np.var(ddof=1) + 1."""
    with np.errstate(all='ignore'):
        return np.var(_species(Y, species), axis=1, ddof=1) + 1


def stock_log_variance(Y, species):
    with np.errstate(all='ignore'):
        return np.log(variance_plus_one(Y, species))


def stock_autocorr(Y, species, lag):
    a = _species(Y, species)
    n_obs = a.shape[1]
    with np.errstate(all='ignore'):
        mu = np.mean(a, axis=1, keepdims=True)
        sd = np.std(a, axis=1, ddof=1, keepdims=True)
        sx = (a - mu) / sd
        return np.sum(sx[:, lag:] * sx[:, :-lag], axis=1) / (n_obs - 1)


def stock_crosscorr(Y):
    a, b = _species(Y, 0), _species(Y, 1)
    n_obs = a.shape[1]
    with np.errstate(all='ignore'):
        sa = (a - np.mean(a, axis=1, keepdims=True)) / np.std(a, axis=1, keepdims=True)      # ddof 0, but / (n_obs - 1)
        sb = (b - np.mean(b, axis=1, keepdims=True)) / np.std(b, axis=1, keepdims=True)
        return np.sum(sa * sb, axis=1) / (n_obs - 1)


def summaries(Y):
    """(n, 9) in the order of NAMES; a constant series gives 0 / 0 = NaN in its correlations, as the example does."""
    return np.column_stack([stock_mean(Y, 0), stock_mean(Y, 1), stock_log_variance(Y, 0), stock_log_variance(Y, 1),
                            stock_autocorr(Y, 0, 1), stock_autocorr(Y, 1, 1), stock_autocorr(Y, 0, 2),
                            stock_autocorr(Y, 1, 2), stock_crosscorr(Y)])


def log_arguments(Y):
    """(n, 2): what the two log-variance columns take the logarithm of."""
    return np.column_stack([variance_plus_one(Y, 0), variance_plus_one(Y, 1)])


def euclidean(S, obs):
    """cdist's euclidean of the rows of S to the observed nine: the square root of the sum of squares in column order."""
    S = np.atleast_2d(np.asarray(S, dtype=np.float64))
    obs = np.asarray(obs, dtype=np.float64).reshape(-1)
    acc = np.zeros(S.shape[0])
    with np.errstate(all='ignore'):
        for j in range(S.shape[1]):
            d = S[:, j] - obs[j]
            acc = acc + d * d
        return np.sqrt(acc)


class Replay:
    """A random_state that replays given draws in the order the reference simulator asks for them: exponential(scale) ->
    scale E[:, k], uniform(size) -> U[:, k], normal(scale, size) -> scale Z[:, q]."""

    def __init__(self, E, U, Z=None):
        self.E, self.U, self.Z = E, U, Z
        self.ke = self.ku = self.q = 0

    def exponential(self, scale):
        self.ke += 1
        with np.errstate(all='ignore'):
            return scale * self.E[:, self.ke - 1]

    def uniform(self, size):
        self.ku += 1
        return self.U[:, self.ku - 1].reshape(size)

    def normal(self, scale=1.0, size=None):
        self.q += 1
        if self.Z is None:
            return np.zeros(size)
        return scale * self.Z[:, self.q - 1]


def golden_draws(seed, batch, n_events, n_obs):
    """(E, U, Z) of a recorded run (scripts/make_golden_lv.py), regenerated from its seed."""
    rs = np.random.RandomState(int(seed))
    return rs.exponential(size=(batch, n_events)), rs.uniform(size=(batch, n_events)), rs.randn(batch, 2 * (n_obs - 1))
