"""NumPy statements of what csrc/romc.hip computes (include/elfihip.h, "ROMC"): the frozen-noise MA2 objective, SciPy's
Nelder-Mead, the difference Hessian, the Jacobi rotation with NumPy's rank rule, the reference's line search, the box
transform of the sampler and the indicator counts.  Written from the algorithms; tests/test_romc.py pins them to SciPy and
to the reference's RegionConstructor, tests/test_romc_gpu.py compares the device with them bit for bit.
"""
import numpy as np

SOLVED, MAXFEV, MAXITER, NONFINITE = range(4)
EPS = np.finfo(np.float64).eps


def make_noise(n1, n_obs, seed):
    return np.random.RandomState(seed).standard_normal((n1, n_obs + 2))


def objective_rows(W, t1, t2, obs):
    """f for rows of noise W (P, n_obs + 2) and parameters t1, t2 (P): D D with D the MA2 example's distance."""
    W = np.atleast_2d(np.asarray(W, dtype=np.float64))
    t1 = np.asarray(t1, dtype=np.float64).reshape(-1, 1)
    t2 = np.asarray(t2, dtype=np.float64).reshape(-1, 1)
    x = np.ascontiguousarray((W[:, 2:] + t1 * W[:, 1:-1]) + t2 * W[:, :-2])
    s1 = np.mean(np.ascontiguousarray(x[:, 1:] * x[:, :-1]), axis=1)
    s2 = np.mean(np.ascontiguousarray(x[:, 2:] * x[:, :-2]), axis=1)
    d1, d2 = s1 - obs[0], s2 - obs[1]
    D = np.sqrt(d1 * d1 + d2 * d2)
    return D * D


def make_objective(w, obs):
    """theta (2,) -> f as a Python float, for one noise row."""
    w = np.asarray(w, dtype=np.float64)

    def f(theta):
        return float(objective_rows(w[None, :], theta[0], theta[1], obs)[0])
    return f


class _Refused(Exception):
    pass


def nelder_mead(f, x0, maxiter=None, maxfev=None, xatol=1e-4, fatol=1e-4):
    """scipy.optimize.minimize(f, x0, method='Nelder-Mead') for a float64 x0 without bounds: (x, fun, nfev, nit, status).
    A value that is not finite ends the problem with status NONFINITE and NaN outputs (the device's rule; SciPy goes on)."""
    x0 = np.asarray(x0, dtype=np.float64).reshape(-1)
    N = len(x0)
    if maxiter is None and maxfev is None:
        maxiter = maxfev = N * 200
    elif maxiter is None:
        maxiter = np.inf
    elif maxfev is None:
        maxfev = np.inf
    sim = np.empty((N + 1, N))
    sim[0] = x0
    for k in range(N):
        y = x0.copy()
        y[k] = (1 + 0.05) * y[k] if y[k] != 0 else 0.00025
        sim[k + 1] = y
    fsim = np.full(N + 1, np.inf)
    state = dict(fev=0, bad=False)

    def call(x):
        if state['fev'] >= maxfev:
            raise _Refused()
        state['fev'] += 1
        v = f(np.copy(x))
        if not np.isfinite(v):
            state['bad'] = True
            raise _Refused()
        return v

    def order():
        ind = np.argsort(fsim, kind='stable')
        return np.take(sim, ind, 0), np.take(fsim, ind, 0)

    try:
        for k in range(N + 1):
            fsim[k] = call(sim[k])
    except _Refused:
        pass
    sim, fsim = order()
    it = 1
    while not state['bad'] and state['fev'] < maxfev and it < maxiter:
        try:
            if np.max(np.ravel(np.abs(sim[1:] - sim[0]))) <= xatol and np.max(np.abs(fsim[0] - fsim[1:])) <= fatol:
                break
            xbar = np.add.reduce(sim[:-1], 0) / N
            xr = 2 * xbar - 1 * sim[-1]
            fxr = call(xr)
            shrink = False
            if fxr < fsim[0]:
                xe = 3 * xbar - 2 * sim[-1]
                fxe = call(xe)
                if fxe < fxr:
                    sim[-1], fsim[-1] = xe, fxe
                else:
                    sim[-1], fsim[-1] = xr, fxr
            elif fxr < fsim[-2]:
                sim[-1], fsim[-1] = xr, fxr
            else:
                if fxr < fsim[-1]:
                    xc = 1.5 * xbar - 0.5 * sim[-1]
                    fxc = call(xc)
                    if fxc <= fxr:
                        sim[-1], fsim[-1] = xc, fxc
                    else:
                        shrink = True
                else:
                    xcc = 0.5 * xbar + 0.5 * sim[-1]
                    fxcc = call(xcc)
                    if fxcc < fsim[-1]:
                        sim[-1], fsim[-1] = xcc, fxcc
                    else:
                        shrink = True
                if shrink:
                    for j in range(1, N + 1):
                        sim[j] = sim[0] + 0.5 * (sim[j] - sim[0])
                        fsim[j] = call(sim[j])
            it += 1
        except _Refused:
            pass
        sim, fsim = order()
    if state['bad']:
        return np.full(N, np.nan), np.nan, state['fev'], it, NONFINITE
    status = MAXFEV if state['fev'] >= maxfev else (MAXITER if it >= maxiter else SOLVED)
    return sim[0].copy(), float(fsim[0]), state['fev'], it, status


def hessian(f, x, f0):
    """Central second differences with the steps h_k = 2^-13 max(1, |x_k|) (D = 2)."""
    x = np.asarray(x, dtype=np.float64)
    h = 2.0 ** -13 * np.maximum(1.0, np.abs(x))
    H = np.empty((2, 2))
    for k in range(2):
        e = np.zeros(2)
        e[k] = h[k]
        H[k, k] = ((f(x + e) - f0) + (f(x - e) - f0)) / (h[k] * h[k])
    pp, pm = f(x + h), f(x + h * [1, -1])
    mp, mm = f(x + h * [-1, 1]), f(x - h)
    H[0, 1] = H[1, 0] = ((pp - pm) - (mp - mm)) / ((4.0 * h[0]) * h[1])
    return H


def solve(W, obs, x0, maxiter=None, maxfev=None):
    """What elfihip_romc_solve returns for noise W (n1, n_obs + 2) and starts x0 (n1, 2), as a dict of arrays."""
    n1 = len(W)
    out = dict(x_min=np.empty((n1, 2)), f_min=np.empty(n1), hess=np.full((n1, 2, 2), np.nan), nfev=np.empty(n1, dtype=np.int32),
               nit=np.empty(n1, dtype=np.int32), status=np.empty(n1, dtype=np.int32))
    for i in range(n1):
        f = make_objective(W[i], obs)
        x, fun, nfev, nit, status = nelder_mead(f, x0[i], maxiter, maxfev)
        out['x_min'][i], out['f_min'][i], out['nfev'][i], out['nit'][i], out['status'][i] = x, fun, nfev, nit, status
        if status == SOLVED:
            out['hess'][i] = hessian(f, x, fun)
    return out


def rotation(H):
    """One Jacobi rotation of the symmetric part of H (2, 2), columns = eigenvectors; the identity when H or an eigenvalue
    is not finite or min |lambda| <= max |lambda| D eps (numpy.linalg.matrix_rank's rule)."""
    H = np.asarray(H, dtype=np.float64)
    eye = np.eye(2)
    if not np.all(np.isfinite(H)):
        return eye
    a, d, b = H[0, 0], H[1, 1], (H[0, 1] + H[1, 0]) * 0.5
    V = eye
    with np.errstate(all='ignore'):
        if b != 0.0:
            tau = (d - a) / (2.0 * b)
            root = np.sqrt(1.0 + tau * tau)
            t = 1.0 / (tau + root) if tau >= 0.0 else -1.0 / (-tau + root)
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = t * c
            a, d = a - t * b, d + t * b
            V = np.array([[c, s], [-s, c]])
        lam = np.abs([a, d])
        if not np.all(np.isfinite(lam)) or lam.min() <= lam.max() * 2 * EPS:
            return eye
    return V


def line_search(f, th_star, vd, eps, K=10, eta=1., rep_lim=300):
    """The reference's line search, operation for operation: (offset, number of evaluations)."""
    th = np.array(th_star, dtype=np.float64)
    offset, evals = 0.0, 0
    for _ in range(K):
        rep = 0
        while True:
            v = f(th)
            evals += 1
            if not (v < eps and rep <= rep_lim):
                break
            th += eta * vd
            offset += eta
            rep += 1
        th -= eta * vd
        offset -= eta
        if rep > rep_lim:
            break
        eta = eta / 2
    if offset <= 0:
        offset = eta
    return offset, evals


def regions(W, obs, prob, centre, hess, eps_region, K=10, eta=1., rep_lim=300):
    """What elfihip_romc_regions returns: rotation (R, 2, 2), limits (R, 2, 2), nfev (R, 2, 2)."""
    R = len(prob)
    out = dict(rotation=np.empty((R, 2, 2)), limits=np.empty((R, 2, 2)), nfev=np.empty((R, 2, 2), dtype=np.int32))
    for r in range(R):
        f = make_objective(W[prob[r]], obs)
        V = rotation(hess[r])
        out['rotation'][r] = V
        for d in range(2):
            lo, n_lo = line_search(f, centre[r], -V[:, d], eps_region, K, eta, rep_lim)
            hi, n_hi = line_search(f, centre[r], V[:, d], eps_region, K, eta, rep_lim)
            out['limits'][r, d] = -lo, hi
            out['nfev'][r, d] = n_lo, n_hi
    return out


def box_transform(u, centre, rot, limits):
    """Uniforms u (n2, 2) -> points of the box: t_k = u_k (hi_k - lo_k) + lo_k, theta_i = (rot[i, 0] t_0 + rot[i, 1] t_1) + c_i."""
    t = u * (limits[:, 1] - limits[:, 0]) + limits[:, 0]
    return np.stack([(rot[0, 0] * t[:, 0] + rot[0, 1] * t[:, 1]) + centre[0],
                     (rot[1, 0] * t[:, 0] + rot[1, 1] * t[:, 1]) + centre[1]], axis=1)


def contains(p, centre, rot_inv, limits):
    """NDimBoundingBox.contains, term by term (D = 2): bool (BS) for points p (BS, 2)."""
    ok = np.ones(len(p), dtype=bool)
    for k in range(2):
        y = (rot_inv[k, 0] * p[:, 0] + rot_inv[k, 1] * p[:, 1]) + (rot_inv[k, 0] * -centre[0] + rot_inv[k, 1] * -centre[1])
        ok &= ~((y < limits[k, 0]) | (y > limits[k, 1]))
    return ok


def count(W, obs, theta, prob, eps, boxes=None):
    """count[b] = sum_r 1[f_{prob[r]}(theta_b) <= eps] (and theta_b in box r with boxes = (centre, rotation_inv, limits))."""
    theta = np.asarray(theta, dtype=np.float64)
    out = np.zeros(len(theta), dtype=np.int32)
    for r, i in enumerate(prob):
        inside = objective_rows(np.broadcast_to(W[i], (len(theta), W.shape[1])), theta[:, 0], theta[:, 1], obs) <= eps
        if boxes is not None:
            inside &= contains(theta, boxes[0][r], boxes[1][r], boxes[2][r])
        out += inside
    return out
