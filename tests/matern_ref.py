"""TEST INFRASTRUCTURE ONLY -- NumPy statement of GP regression under a stationary kernel of one of three kinds plus a
bias: [GPy-upstream] kern.RBF / kern.Matern32 / kern.Matern52 (each optionally ARD=True) + kern.Bias under
ExactGaussianInference.

No reference fixture exists for the Matern kernels (GPy is not installed where the fixtures are recorded), so this file is
the statement the Matern tests compare with; tests/test_gp_matern.py checks it against mpmath and against central
differences of its own values.  With a = r / l (r2 = sum_c (x_c - x'_c)^2 / l_c^2 for per-dimension lengthscales):

    kind       k(r2)                                        g(r2) = dk / d(r2)
    rbf        s_f exp(-r2 / 2l^2)                          -k / (2l^2)
    matern32   s_f (1 + sqrt3 a) exp(-sqrt3 a)              -(3 / 2l^2) s_f exp(-sqrt3 a)
    matern52   s_f (1 + sqrt5 a + 5 a^2 / 3) exp(-sqrt5 a)  -(5 / 6l^2) s_f (1 + sqrt5 a) exp(-sqrt5 a)

    grad_x k = 2 g (x - X),   dk/dl = -2 g r2 / l,   per dimension  dk/dl_c = -2 g D_c^2 / l_c
    (D_c = x_c - X_c; with per-dimension lengthscales g is taken w.r.t. the SCALED r2 and D_c^2 / l_c^3 takes its place)

g is finite at r = 0 for every kind; nothing here divides by r.  The posterior follows oracle/gp_oracle.py's Posterior and
tests/ard_ref.py's ArdPosterior, which MaternPosterior equals for kind 'rbf':

    Ky = K + s_b + (s_n + 1e-8) I,  log Z = 0.5 (-n log 2 pi - log det Ky - y' alpha),  dL/dK = 0.5 (alpha alpha' - Ky^-1)
    d log Z / d s_f = sum(dL/dK * K_st) / s_f,  d log Z / d l_c = sum(dL/dK * dK_st/dl_c),
    d log Z / d s_b = sum(dL/dK),  d log Z / d s_n = trace(dL/dK)
    mean(x) = k(x)' alpha,  var(x) = max(s_f + s_b - k(x)' Ky^-1 k(x), 1e-15) [+ s_n]

Squared distances are formed from DIFFERENCES (exact to rounding however close two rows lie).  `kern_gpy` alone forms them as
GPy's Stationary._unscaled_dist does -- (|a|^2 + |b|^2) - 2 a.b clipped at 0 -- and so carries that form's cancellation
error for nearly coincident rows: the tests of the device's kernel matrix bound the device by 16 x the error of `kern_gpy`
against mpmath on the same inputs.
"""
import numpy as np
import scipy.linalg as sl

JITTER = 1e-8
KINDS = ('rbf', 'matern32', 'matern52')
SQRT3, SQRT5 = np.sqrt(3.0), np.sqrt(5.0)


def kg(kind, r2, var=1.0, ls=1.0):
    """(k, g = dk/d(r2)) at squared distances r2 >= 0 (any shape) for signal variance var and lengthscale ls."""
    r2 = np.asarray(r2, dtype=float)
    l2 = float(ls) ** 2
    if kind == 'rbf':
        k = var * np.exp(-0.5 * r2 / l2)
        return k, -k / (2.0 * l2)
    a = np.sqrt(r2 / l2)
    if kind == 'matern32':
        e = var * np.exp(-SQRT3 * a)
        return (1.0 + SQRT3 * a) * e, -(3.0 / (2.0 * l2)) * e
    if kind == 'matern52':
        e = var * np.exp(-SQRT5 * a)
        return (1.0 + SQRT5 * a + 5.0 * a * a / 3.0) * e, -(5.0 / (6.0 * l2)) * (1.0 + SQRT5 * a) * e
    raise ValueError(kind)


def scaled_r2(A, B, ell):
    """(len(A), len(B)) squared distances sum_c (A_ic - B_jc)^2 / l_c^2, one dimension at a time, differences first."""
    r2 = np.zeros((A.shape[0], B.shape[0]))
    for c in range(A.shape[1]):
        diff = A[:, c, None] - B[None, :, c]
        r2 += diff * diff / ell[c] ** 2
    return r2


def gpy_r2(A, B=None):
    """[GPy-upstream] Stationary._unscaled_dist squared: (|a|^2 + |b|^2) - 2 a.b clipped at 0, exactly 0 on the diagonal when
    B is None."""
    if B is None:
        sq = np.sum(np.square(A), 1)
        r2 = -2.0 * A.dot(A.T) + (sq[:, None] + sq[None, :])
        r2[np.diag_indices_from(r2)] = 0.0
    else:
        r2 = -2.0 * A.dot(B.T) + (np.sum(np.square(A), 1)[:, None] + np.sum(np.square(B), 1)[None, :])
    return np.clip(r2, 0.0, np.inf)


def kern_gpy(kind, A, B, var, ls, bias):
    """Prior covariance k(A, B) (k(A, A) when B is None) with r2 formed the way GPy forms it; one lengthscale."""
    return kg(kind, gpy_r2(A, B), var, ls)[0] + bias


def log_marginal(X, Y, kind, var, ell, bias, noise):
    return MaternPosterior(X, Y, kind, var, ell, bias, noise, need_inv=False).log_marginal


class MaternPosterior:
    """ell: one lengthscale, or one per input dimension."""

    def __init__(self, X, Y, kind, var, ell, bias, noise, need_inv=True):
        self.kind = kind
        self.X = np.asarray(X, dtype=float)
        self.Y = np.asarray(Y, dtype=float).reshape(-1, 1)
        n, d = self.X.shape
        self.ell = np.broadcast_to(np.asarray(ell, dtype=float).reshape(-1), (d,)).copy()
        self.var, self.bias, self.noise = float(var), float(bias), float(noise)
        self.Kst, self.G = kg(kind, scaled_r2(self.X, self.X, self.ell), self.var)    # g w.r.t. the scaled r2
        Ky = self.Kst + self.bias
        Ky[np.diag_indices(n)] += self.noise + JITTER
        self.L = sl.cholesky(Ky, lower=True)
        self.alpha = sl.cho_solve((self.L, True), self.Y)
        self.log_marginal = 0.5 * (-n * np.log(2 * np.pi) - 2. * np.sum(np.log(np.diag(self.L)))
                                   - float((self.Y.T @ self.alpha)[0, 0]))
        if need_inv:
            Linv = sl.solve_triangular(self.L, np.eye(n), lower=True)
            self.Kinv = Linv.T @ Linv

    def _x(self, x):
        return np.asarray(x, dtype=float).reshape(-1, self.X.shape[1])

    def kern(self, A, B):
        """Prior covariance k(A, B)."""
        return kg(self.kind, scaled_r2(self._x(A), self._x(B), self.ell), self.var)[0] + self.bias

    def log_marginal_grad(self, isotropic=False):
        """d log Z / d (var, l_1 .. l_d, bias, noise) -- GPy's param_array order; isotropic: (var, l, bias, noise) for the one
        lengthscale all dimensions share (the sum of the per-dimension derivatives)."""
        D = 0.5 * (self.alpha @ self.alpha.T - self.Kinv)
        E = D * self.G
        g_ell = np.empty(self.X.shape[1])
        for c in range(self.X.shape[1]):
            diff = self.X[:, c, None] - self.X[None, :, c]
            g_ell[c] = np.sum(E * (-2.0 * diff * diff)) / self.ell[c] ** 3
        if isotropic:
            g_ell = np.array([g_ell.sum()])
        return np.concatenate([[np.sum(D * self.Kst) / self.var], g_ell, [np.sum(D), np.trace(D)]])

    def predict(self, x, noiseless=False):
        Kx = self.kern(self.X, x)                                                # (n, S)
        mu = Kx.T @ self.alpha
        v = np.clip((self.var + self.bias) - np.sum((self.Kinv @ Kx) * Kx, 0), 1e-15, np.inf)[:, None]
        return mu, v if noiseless else v + self.noise

    def dk_dx(self, x):
        """(S, n, d): derivative of the stationary part k(x_s, X_i) w.r.t. x_s -- 2 g (x - X) / l_c^2, finite at x = X_i."""
        x = self._x(x)
        g = kg(self.kind, scaled_r2(x, self.X, self.ell), self.var)[1]
        return 2.0 * g[:, :, None] * (x[:, None, :] - self.X[None, :, :]) / self.ell ** 2

    def predictive_gradients(self, x):
        dk = self.dk_dx(x)
        Kx = self.kern(x, self.X)                                                # (S, n)
        return (np.einsum('snd,n->sd', dk, self.alpha[:, 0]), np.einsum('snd,sn->sd', dk, -2. * Kx @ self.Kinv))

    def cross_cov(self, P, x):
        """Posterior covariance (M, S) between the rows of P and of x."""
        return self.kern(P, x) - self.kern(P, self.X) @ self.Kinv @ self.kern(self.X, x)

    def lcb(self, x, beta):
        """(value (S, 1), gradient (S, d)) of mean - sqrt(beta var), noiseless variance (acquisition.py:256-301)."""
        mu, v = self.predict(x, noiseless=True)
        gm, gv = self.predictive_gradients(x)
        return mu - np.sqrt(beta * v), gm - 0.5 * gv * np.sqrt(beta / v)


# ---- 40-digit evaluation (mpmath) of k and g, and of a kernel matrix from the float coordinates themselves --------------
def _kg_mp(mp, kind, r2, var, l2):
    """(k, g) from mpmath numbers, inside the caller's working precision."""
    if kind == 'rbf':
        k = var * mp.exp(-r2 / (2 * l2))
        return k, -k / (2 * l2)
    a = mp.sqrt(r2 / l2)
    if kind == 'matern32':
        e = var * mp.exp(-mp.sqrt(3) * a)
        return (1 + mp.sqrt(3) * a) * e, -(3 / (2 * l2)) * e
    e = var * mp.exp(-mp.sqrt(5) * a)
    return (1 + mp.sqrt(5) * a + 5 * a * a / 3) * e, -(5 / (6 * l2)) * (1 + mp.sqrt(5) * a) * e


def kg_mp(kind, r2, var=1.0, ls=1.0, dps=40):
    """(k, g) at ONE float r2 as mpmath numbers of `dps` digits: every input is taken as the exact binary number it is."""
    import mpmath as mp
    with mp.workdps(dps):
        return _kg_mp(mp, kind, mp.mpf(float(r2)), mp.mpf(float(var)), mp.mpf(float(ls)) ** 2)


def kern_mp(kind, A, B, var, ls, bias, dps=40):
    """k(A, B) + bias with the squared distances formed exactly from the float coordinates, rounded to float at the end."""
    import mpmath as mp
    A, B = np.asarray(A, float), np.asarray(B, float)
    out = np.empty((A.shape[0], B.shape[0]))
    with mp.workdps(dps):
        for i in range(A.shape[0]):
            for j in range(B.shape[0]):
                r2 = mp.fsum((mp.mpf(float(a)) - mp.mpf(float(b))) ** 2 for a, b in zip(A[i], B[j]))
                k = _kg_mp(mp, kind, r2, mp.mpf(float(var)), mp.mpf(float(ls)) ** 2)[0]
                out[i, j] = float(k + mp.mpf(float(bias)))
    return out
