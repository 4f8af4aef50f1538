"""NumPy statement of the day-care-centre transmission model the device runs (csrc/daycare.hip): Gillespie's direct method
for the carriage of n_strains strains by the n_ind individuals of a centre (Numminen et al. 2013; elfi/examples/daycare.py),
the four summaries over the first n_obs individuals and the example's sorted L1 distance.

Every (simulation, centre) pair is a row of its own: it stops at ITS first event at or past time_end.  The reference keeps
every centre of every simulation of a batch jumping until the slowest has passed time_end, so it is reproduced exactly only
with batch_size = 1, n_dcc = 1 -- which is how tests/golden/daycare.npz was recorded (scripts/make_golden_daycare.py).

The hazard of (individual i, strain s) is 1 where i carries s, else c_i g_s with
    P_s = sum_i I_is / k_i  (k_i strains carried by i; i ascending, from 0),  g_s = ((t1 P_s) nf + 1e-9) + t2 f_s,  nf = 1 / (n_ind - 1)
    c_i = t3 if k_i > 0 else 1
Rows are summed over s ascending, the rows over i ascending (np.cumsum: strictly left to right), the event is chosen by
target = u total: the first individual whose cumulative row sum exceeds it, then the first strain whose partial row sum exceeds
target minus the cumulative sum before that individual.  The reference sums all n_ind n_strains hazards pairwise and compares
u to cumsum(hazards / total): the same choice unless u lies within rounding (1e-13) of a boundary; the recorder keeps 1e-9.
"""
import numpy as np

import philox_ref as P

EPS = np.finfo(np.float64).eps
NAMES = ('Shannon', 'n_strains', 'prevalence', 'multi')
REACHED_END, OUT_OF_EVENTS, INVALID = 0, 1, 2
MAX_EVENTS = 1 << 21
EVENT_BITS = 22                  # Philox counter word 0 of the drawn form: (centre << 22) | event


def _col(t, batch):
    return np.array(np.broadcast_to(np.asarray(t, dtype=np.float64).reshape(-1), (batch,)))


def simulate(t1, t2, t3, E, U, n_ind=53, n_strains=33, freq_strains_commun=None, n_obs=36, time_end=10.):
    """(state (n, n_dcc, n_obs, n_strains) bool, t_final (n, n_dcc), status (n, n_dcc) int32, events (n, n_dcc) int64) from given
    draws E, U (n, n_dcc, n_events): column k - 1 feeds event k, max_events = n_events."""
    E, U = np.asarray(E, dtype=np.float64), np.asarray(U, dtype=np.float64)
    n, n_dcc, max_events = E.shape
    R = n * n_dcc
    E, U = E.reshape(R, max_events), U.reshape(R, max_events)
    f = np.full(n_strains, 0.1) if freq_strains_commun is None else np.asarray(freq_strains_commun, dtype=np.float64).reshape(-1)
    t1, t2, t3 = (np.repeat(_col(t, n), n_dcc) for t in (t1, t2, t3))
    nf = 1.0 / (n_ind - 1)
    with np.errstate(all='ignore'):
        valid = np.isfinite(t1) & (t1 >= 0) & np.isfinite(t2) & (t2 >= 0) & np.isfinite(t3) & (t3 >= 0)
        state = np.zeros((R, n_ind, n_strains), dtype=bool)
        t = np.zeros(R)
        events = np.zeros(R, dtype=np.int64)
        status = np.full(R, OUT_OF_EVENTS, dtype=np.int32)
        status[~valid] = INVALID
        live = valid.copy()
        t2f = t2[:, None] * f[None, :]
        for k in range(1, max_events + 1):
            L = np.flatnonzero(live)
            if L.size == 0:
                break
            st = state[L]
            cnt = st.sum(axis=2)
            invk = np.where(cnt > 0, 1.0 / np.maximum(cnt, 1), 0.0)
            Ps = np.cumsum(np.where(st, invk[:, :, None], 0.0), axis=1)[:, -1, :]
            g = ((t1[L, None] * Ps) * nf + 1e-9) + t2f[L]
            c = np.where(cnt > 0, t3[L, None], 1.0)
            h = np.where(st, 1.0, c[:, :, None] * g[:, None, :])
            rowcum = np.cumsum(h, axis=2)
            cum = np.cumsum(rowcum[:, :, -1], axis=1)
            total = cum[:, -1]
            t_new = t[L] + E[L, k - 1] / total
            target = U[L, k - 1] * total
            a = np.arange(L.size)
            i_star = np.sum(target[:, None] >= cum[:, :-1], axis=1)
            prev = np.where(i_star > 0, cum[a, np.maximum(i_star - 1, 0)], 0.0)
            rem = target - prev
            s_star = np.sum(rem[:, None] >= rowcum[a, i_star, :-1], axis=1)
            state[L, i_star, s_star] ^= True
            t[L] = t_new
            events[L] = k
            done = t_new >= time_end
            status[L[done]] = REACHED_END
            live[L[done]] = False
        t[~valid] = np.nan
    shape = (n, n_dcc)
    return state[:, :n_obs, :].reshape(shape + (n_obs, n_strains)), t.reshape(shape), status.reshape(shape), events.reshape(shape)


def draws(seed, stream, n, n_dcc, n_events, first=0):
    """(E, U, A), each (n, n_dcc, n_events): event k of centre c of simulation i reads Philox counter words ((c << 22) | k,
    first + i, stream low, stream high) under key seed; E = -log((a + 1) 2^-53) with a the 53 bits of words 0, 1 (A, returned
    for the ulp comparison), U = the 53 bits of words 2, 3 times 2^-53."""
    u64 = np.uint64
    i = (np.arange(n, dtype=u64) + u64(first))[:, None, None]
    c = np.arange(n_dcc, dtype=u64)[None, :, None]
    k = np.arange(1, n_events + 1, dtype=u64)[None, None, :]
    c0, c1 = np.broadcast_arrays((c << u64(EVENT_BITS)) | k, i)
    lo, s32 = u64(0xffffffff), u64(32)
    seed, stream = u64(int(seed) & (2 ** 64 - 1)), u64(int(stream) & (2 ** 64 - 1))
    zero = np.zeros_like(c0)
    r = P.philox4x32_10_vec((c0.copy(), c1.copy(), zero + (stream & lo), zero + (stream >> s32)), (seed & lo, seed >> s32))
    a = (r[0] << u64(21)) | (r[1] >> u64(11))
    b = (r[2] << u64(21)) | (r[3] >> u64(11))
    A = (a + u64(1)).astype(np.float64) * 2.0 ** -53
    return -np.log(A), b.astype(np.float64) * 2.0 ** -53, A


# ---- the four summaries (elfi/examples/daycare.py: ss_shannon, ss_strains, ss_prevalence, ss_prevalence_multi) ----------------
def proportions(state):
    """(n, n_dcc, n_strains): the share of each strain among the observed carriages, 0 / 0 -> 0, then 0 -> 1."""
    total_obs = np.sum(state, axis=2)
    with np.errstate(all='ignore'):
        p = np.nan_to_num(total_obs / np.sum(total_obs, axis=2, keepdims=True))
    p[p == 0] = 1
    return p


def ss_shannon(state):
    p = np.ascontiguousarray(proportions(state))
    return -np.sum(p * np.log(p), axis=2)


def ss_strains(state):
    return np.sum(np.any(state, axis=2), axis=2)


def ss_prevalence(state):
    return np.sum(np.any(state, axis=3), axis=2) / state.shape[2]


def ss_prevalence_multi(state):
    return np.sum(np.sum(state, axis=3) > 1, axis=2) / state.shape[2]


def summaries(state, status=None):
    """(n, 4, n_dcc) in the order of NAMES; NaN where the centre is not REACHED_END."""
    state = np.asarray(state, dtype=bool)
    S = np.stack([ss_shannon(state), ss_strains(state), ss_prevalence(state), ss_prevalence_multi(state)], axis=1).astype(np.float64)
    if status is not None:
        S[np.broadcast_to((np.asarray(status) != REACHED_END)[:, None, :], S.shape)] = np.nan
    return S


def shannon_bound(state, ulp=4):
    """The largest distance of a Shannon index made with logarithms within `ulp` ulp of np.log from ss_shannon.  A term p log p
    moves by at most ulp eps |p log p| through its logarithm and by eps |p log p| through the rounding of the two products;
    both sums add their n_strains terms in the same order and round each of the n_strains - 1 additions by at most eps / 2
    times a partial sum, which the sum of the |terms| bounds (they have one sign)."""
    p = proportions(np.asarray(state, dtype=bool))
    terms = np.abs(p * np.log(p))
    total = np.sum(terms, axis=2)
    return ((ulp + 1) * EPS * (1 + EPS) + (p.shape[2] - 1) * EPS * (1 + 8 * EPS)) * total


def distance(S, observed):
    """The example's distance of S (n, k, m) to observed (k, m): both divided by the observed row maximum (1 where that is 0),
    each row sorted, |x - y| summed left to right per row and the rows' sums in order, divided by k m.  NaN in, NaN out."""
    S = np.asarray(S, dtype=np.float64)
    obs = np.asarray(observed, dtype=np.float64).reshape(S.shape[1], S.shape[2])
    n, k, m = S.shape
    om = np.max(obs, axis=1, keepdims=True)
    om = np.where(om == 0, 1, om)
    with np.errstate(all='ignore'):
        y = np.sort(obs / om, axis=1)
        x = np.sort(S / om[None], axis=2)
        rows = np.cumsum(np.abs(x - y[None]), axis=2)[:, :, -1]
        return np.cumsum(rows, axis=1)[:, -1] / (k * m)


class Replay:
    """A random_state that replays given draws E, U (batch, n_dcc, n_events) in the order the reference simulator asks for
    them: exponential(scale) -> scale E[:, :, k], uniform(size) -> U[:, :, k]."""

    def __init__(self, E, U):
        self.E, self.U = E, U
        self.ke = self.ku = 0

    def exponential(self, scale):
        self.ke += 1
        return scale * self.E[:, :, self.ke - 1]

    def uniform(self, size):
        self.ku += 1
        return self.U[:, :, self.ku - 1].reshape(size)


def golden_draws(seed, n_dcc, n_events):
    """(E, U), each (n_dcc, n_events), of a recorded set (scripts/make_golden_daycare.py), regenerated from its seed: row c
    feeds centre c, which was recorded as a reference call of its own."""
    rs = np.random.RandomState(int(seed))
    return rs.exponential(size=(n_dcc, n_events)), rs.uniform(size=(n_dcc, n_events))
