"""NumPy statement of the stochastic Lorenz-96 forecast model (ELFI's elfi/examples/lorenz.py) and its six summaries --
what csrc/lorenz.hip computes, written from the formulas in DESIGN.md ("The Lorenz-96 example model"), and the same
summaries once more with every summation order spelled out in plain Python (the orders the kernel implements).

    X = lorenz_series(theta1, theta2, E, y0, f, c, phi, h)       (B, T, K); E: (B, T - 1, K) standard normals
    S = lorenz_summaries(X)                                       (B, 6): Mean, Var, Autocov, Cov, CrosscovPrev, CrosscovNext
    S = lorenz_summaries_explicit(X)                              the same numbers, sums in explicit order
"""
import numpy as np

NAMES = ['Mean', 'Var', 'Autocov', 'Cov', 'CrosscovPrev', 'CrosscovNext']


def lorenz_constants(phi=0.984, n_timestep=160, total_duration=4):
    """c = sqrt(1 - phi^2) and the time step h, as Python computes them on the host."""
    return float(np.sqrt(1 - pow(phi, 2))), total_duration / n_timestep


def lorenz_noise_from_state(rs, B, T, K):
    """The draws the reference's simulator consumes: one normal(0, 1, (B, K)) per step 1 .. T - 1, stacked to (B, T - 1, K)."""
    if T < 2:
        return np.empty((B, 0, K))
    return np.stack([rs.normal(0, 1, (B, K)) for _ in range(1, T)], axis=1)


def lorenz_series(theta1, theta2, E, y0, f=10., c=None, phi=0.984, h=None):
    E = np.asarray(E, dtype=np.float64)
    B, K = E.shape[0], E.shape[2]
    T = E.shape[1] + 1
    if c is None:
        c = lorenz_constants(phi, T)[0]
    if h is None:
        h = lorenz_constants(phi, T)[1]
    th1 = np.broadcast_to(np.asarray(theta1, dtype=np.float64).reshape(-1), (B,)).reshape(B, 1)
    th2 = np.broadcast_to(np.asarray(theta2, dtype=np.float64).reshape(-1), (B,)).reshape(B, 1)
    y = np.array(np.broadcast_to(np.asarray(y0, dtype=np.float64), (B, K)))
    X = np.empty((B, T, K))
    X[:, 0] = y
    eta = np.zeros((B, K))

    def ode(y):
        ym2, ym1, yp1 = np.roll(y, 2, axis=1), np.roll(y, 1, axis=1), np.roll(y, -1, axis=1)
        g = th1 + y * th2
        return ((((-ym2 * ym1 + ym1 * yp1) - y) + f) - g) + eta

    with np.errstate(all='ignore'):
        for i in range(1, T):
            eta = phi * eta + E[:, i - 1] * c
            k1 = h * ode(y)
            k2 = h * ode(y + k1 / 2)
            k3 = h * ode(y + k2 / 2)
            k4 = h * ode(y + k3)
            y = y + (((k1 + 2 * k2) + 2 * k3) + k4) / 6
            X[:, i] = y
    return X


def lorenz_summaries(X):
    X = np.asarray(X, dtype=np.float64)
    with np.errstate(all='ignore'):
        nxt, prv = np.roll(X, -1, axis=2), np.roll(X, 1, axis=2)
        head = X[:, :-1] - np.mean(X[:, :-1], keepdims=True, axis=1)

        def lagged(Z):
            return np.mean(head * (Z[:, 1:] - np.mean(Z[:, 1:], keepdims=True, axis=1)), axis=(1, 2))

        cov = np.mean(np.mean((X - np.mean(X, keepdims=True, axis=1)) * (nxt - np.mean(nxt, keepdims=True, axis=1)), axis=1),
                      axis=1)
        return np.column_stack([np.mean(X, axis=(1, 2)), np.mean(np.var(X, axis=1), axis=1), lagged(X), cov, lagged(prv),
                                lagged(nxt)])


# ---- the same with every order spelled out ------------------------------------------------------------------------------
def pairwise_block(a):
    """NumPy's sum of at most 128 terms: in order below 8, else eight interleaved accumulators and the tail in order."""
    n = len(a)
    if n < 8:
        r = 0.0
        for v in a:
            r = r + v
        return r
    r = [a[j] for j in range(8)]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = r[j] + a[i + j]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        res = res + v
    return res


def pairwise(a):
    """NumPy's pairwise sum of a contiguous run (at most the 8192 terms of one reduction buffer)."""
    n = len(a)
    if n <= 128:
        return pairwise_block(a)
    n2 = n // 2
    n2 -= n2 % 8
    return pairwise(a[:n2]) + pairwise(a[n2:])


def seq(a):
    """Left-to-right sum along axis 0."""
    r = np.array(a[0], dtype=np.float64)
    for row in a[1:]:
        r = r + row
    return r


def lorenz_summaries_explicit(X):
    X = np.asarray(X, dtype=np.float64)
    out = np.empty((X.shape[0], 6))
    with np.errstate(all='ignore'):
        for s, x in enumerate(X):
            T, K = x.shape
            m = seq(x) / T
            a, b = seq(x[:-1]) / (T - 1), seq(x[1:]) / (T - 1)
            d = x - m
            v = seq(d * d) / T
            q = seq(d * np.roll(d, -1, axis=1)) / T
            head = x[:-1] - a
            tail = x[1:] - b
            out[s, 0] = pairwise(list(x.reshape(-1))) / (T * K)
            out[s, 1] = pairwise(list(v)) / K
            out[s, 2] = pairwise(list((head * tail).reshape(-1))) / ((T - 1) * K)
            out[s, 3] = pairwise(list(q)) / K
            out[s, 4] = pairwise(list((head * np.roll(tail, 1, axis=1)).reshape(-1))) / ((T - 1) * K)
            out[s, 5] = pairwise(list((head * np.roll(tail, -1, axis=1)).reshape(-1))) / ((T - 1) * K)
    return out
