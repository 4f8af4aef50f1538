"""The birth-death-mutation example (elfi/examples/bdm.py, the simulator of its cpp/bdm.cpp) stated in NumPy: what
csrc/bdm.hip computes, operation for operation (include/elfihip.h: elfihip_bdm_clusters), and the uniforms the reference
binary consumes, so that its recorded runs (tests/golden/bdm.npz, scripts/make_golden_bdm.py) can be replayed.

The binary draws from std::mt19937(seed) through std::uniform_real_distribution<double>, which takes two 32-bit words r0, r1
per uniform: u = (r0 + r1 2^32) / 2^64, the sum rounded to a double before the division, and a value that rounds to 1.0
replaced by the largest double below 1.  It keeps ONE generator for all rows of an input file, so simulation i starts where
i - 1 stopped; `replay` walks that stream and cuts it into the per-simulation rows the device's given form takes.
"""
import numpy as np

import philox_ref as P

REACHED_N, EXTINCT, OUT_OF_EVENTS, INVALID = 0, 1, 2, 3
MAX_N = 4096


def mt_uniforms(seed, count):
    """The first `count` doubles std::uniform_real_distribution<double>(0, 1) makes from std::mt19937(seed)."""
    bg = np.random.MT19937()
    bg._legacy_seeding(int(seed))
    raw = bg.random_raw(2 * int(count)).astype(np.float64)
    u = (raw[0::2] + raw[1::2] * 2.0 ** 32) / 2.0 ** 64
    u[u >= 1.0] = np.nextafter(1.0, 0.0)
    return u


def _rate_ok(r):
    return r >= 0.0 and r < np.inf            # False for NaN


def simulate_one(alpha, delta, tau, N, mode, u, max_events=None):
    """One simulation on the uniforms u (ue_1, uc_1, ue_2, uc_2, ...): clusters (N,) int64, status, events, and whether a
    mutation opened a slot that a death had freed (for the golden file's coverage).  max_events None: len(u) // 2."""
    N, mode = int(N), int(mode)
    alpha, delta, tau = np.float64(alpha), np.float64(delta), np.float64(tau)
    u = np.asarray(u, dtype=np.float64)
    if max_events is None:
        max_events = len(u) // 2
    clusters = np.zeros(N, dtype=np.int64)
    with np.errstate(all='ignore'):
        c0 = np.float64(0.0) + alpha
        c1 = c0 + delta
        c2 = c1 + tau
    tot = c2
    if not (_rate_ok(alpha) and _rate_ok(delta) and _rate_ok(tau) and tot > 0.0 and tot < np.inf):
        return clusters, INVALID, 0, False
    clusters[0] = 1
    pop, cend, cap = 1, 1, N + (1 if mode == 1 else 0)
    k, status, cluster, event = 0, REACHED_N, 0, -1
    freed = np.zeros(N, dtype=bool)           # slots emptied by a death
    reopened = False
    while 0 < pop < cap:
        if k == max_events:
            status = OUT_OF_EVENTS
            break
        ue, uc = u[2 * k], u[2 * k + 1]
        if not (0.0 <= ue < 1.0) or not (0.0 <= uc < 1.0):
            return np.zeros(N, dtype=np.int64), INVALID, k, False
        k += 1
        te = ue * tot
        event = 0 if c0 > te else (1 if c1 > te else 2)
        thr = uc * np.float64(pop)
        cum = np.cumsum(clusters[:cend])
        hit = np.nonzero(cum.astype(np.float64) > thr)[0]
        cluster = int(hit[0]) if len(hit) else cend - 1
        if event == 0:
            clusters[cluster] += 1
            pop += 1
        elif event == 1:
            clusters[cluster] -= 1
            pop -= 1
            if clusters[cluster] == 0:
                freed[cluster] = True
        elif clusters[cluster] > 1:
            clusters[cluster] -= 1
            empty = np.nonzero(clusters == 0)[0]
            if len(empty):
                j = int(empty[0])
                clusters[j] = 1
                reopened = reopened or bool(freed[j])
                freed[j] = False
                cend = max(cend, j + 1)
    if status == REACHED_N:
        if pop == 0:
            status = EXTINCT
        elif mode == 1 and k > 0:             # the birth that reached N + 1 is taken back
            clusters[cluster] -= 1
    return clusters, status, k, reopened


def simulate(alpha, delta, tau, N, mode, U, max_events=None):
    """The given form: U (n, 2 n_events).  Returns clusters (n, N) int32, status (n,) int32, events (n,) int64."""
    U = np.atleast_2d(np.asarray(U, dtype=np.float64))
    n = U.shape[0]
    alpha, delta, tau = (np.broadcast_to(np.asarray(t, dtype=np.float64).reshape(-1), (n,)) for t in (alpha, delta, tau))
    Cl, st, ev = np.zeros((n, int(N)), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    for i in range(n):
        Cl[i], st[i], ev[i], _ = simulate_one(alpha[i], delta[i], tau[i], N, mode, U[i], max_events)
    return Cl, st, ev


def replay(params, N, mode, seed, n_events):
    """The reference binary on an input file of the rows (alpha, delta, tau) with population size N: one generator for the
    whole file.  Returns clusters (n, N), status, events, reopened (n,) bool and U (n, 2 n_events): each simulation's own
    stretch of the stream, zero past the draws it used.  A row that is still running after n_events events raises."""
    params = np.atleast_2d(np.asarray(params, dtype=np.float64))
    n = params.shape[0]
    stream = mt_uniforms(seed, 2 * n_events * n)
    at = 0
    Cl, st, ev = np.zeros((n, int(N)), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
    reopened, U = np.zeros(n, dtype=bool), np.zeros((n, 2 * n_events))
    for i, (a, d, t) in enumerate(params):
        Cl[i], st[i], ev[i], reopened[i] = simulate_one(a, d, t, N, mode, stream[at:at + 2 * n_events])
        if st[i] >= OUT_OF_EVENTS:
            raise ValueError('row %d needs more than %d events' % (i, n_events))
        U[i, :2 * ev[i]] = stream[at:at + 2 * ev[i]]
        at += 2 * int(ev[i])
    return Cl, st, ev, reopened, U


def draws(seed, stream, n, n_events, first=0):
    """U (n, 2 n_events) of the drawn form: event k of simulation i reads Philox counter ((first + i) << 32) | k of (seed,
    stream); ue = the 53 bits of words 0, 1 times 2^-53, uc = those of words 2, 3."""
    u64 = np.uint64
    i = (np.arange(n, dtype=u64) + u64(first))[:, None]
    k = np.arange(1, n_events + 1, dtype=u64)[None, :]
    c0, c1 = np.broadcast_arrays(k, i)
    lo, s32 = u64(0xffffffff), u64(32)
    seed, stream = u64(int(seed) & (2 ** 64 - 1)), u64(int(stream) & (2 ** 64 - 1))
    zero = np.zeros_like(c0)
    r = P.philox4x32_10_vec((c0.copy(), c1.copy(), zero + (stream & lo), zero + (stream >> s32)), (seed & lo, seed >> s32))
    U = np.empty((n, 2 * n_events))
    U[:, 0::2] = ((r[0] << u64(21)) | (r[1] >> u64(11))).astype(np.float64) * 2.0 ** -53
    U[:, 1::2] = ((r[2] << u64(21)) | (r[3] >> u64(11))).astype(np.float64) * 2.0 ** -53
    return U


def T1(clusters):
    """elfi/examples/bdm.py: T1, restated."""
    clusters = np.atleast_2d(clusters)
    with np.errstate(all='ignore'):
        return np.sum(clusters > 0, axis=1) / np.sum(clusters, axis=1)


def T2(clusters, n=20):
    """elfi/examples/bdm.py: T2, restated."""
    clusters = np.atleast_2d(clusters)
    return 1 - np.sum((clusters / n) ** 2, axis=1)


def summaries(clusters, status, t2_n):
    """T (n, 2) as the device returns it: T1 and T2 of the clusters, NaN for a simulation cut off or invalid."""
    clusters = np.ascontiguousarray(np.atleast_2d(clusters))
    T = np.column_stack([T1(clusters), T2(clusters, np.float64(t2_n))])
    T[np.asarray(status) >= OUT_OF_EVENTS] = np.nan
    return T


def distance(T, obs):
    """The example's minkowski p = 1 on T1."""
    return np.abs(np.asarray(T)[:, 0] - np.float64(obs))
