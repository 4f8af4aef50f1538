"""TEST INFRASTRUCTURE ONLY -- NumPy statement of GP regression under an RBF kernel with one lengthscale per input dimension
(ARD) plus a bias: [GPy-upstream] kern.RBF(input_dim, ARD=True) + kern.Bias under ExactGaussianInference.

No reference fixture exists for this kernel (GPy is not installed where the fixtures are recorded), so this file is the
statement the ARD tests compare with.  It is independent of the product's way of getting there: K is built from the
per-dimension lengthscales DIRECTLY,

    r2_ij = sum_c (X_ic - X_jc)^2 / l_c^2         (differences first, no |x|^2 + |x'|^2 - 2 x.x' expansion)
    K     = s_f exp(-r2 / 2) + s_b,   Ky = K + (s_n + 1e-8) I

never through inputs divided by l (which is what elfi_amd.gp.ScaledGPHandle does).  Everything else follows
oracle/gp_oracle.py's Posterior, which this class equals when all l_c are equal (tests/test_gp_ard.py):

    log Z = 0.5 (-n log 2 pi - log det Ky - y' alpha),  dL/dK = 0.5 (alpha alpha' - Ky^-1)
    d log Z / d s_f = sum(dL/dK * K_rbf) / s_f,   d log Z / d l_c = sum(dL/dK * K_rbf * (X_ic - X_jc)^2) / l_c^3
    d log Z / d s_b = sum(dL/dK),                 d log Z / d s_n = trace(dL/dK)
    mean(x) = k(x)' alpha,  var(x) = max(s_f + s_b - k(x)' Ky^-1 k(x), 1e-15) [+ s_n]
    d k_i / d x_c = -K_rbf(x, X_i) (x_c - X_ic) / l_c^2
"""
import numpy as np
import scipy.linalg as sl

JITTER = 1e-8


def ard_r2(A, B, ell):
    """(len(A), len(B)) scaled squared distances, one dimension at a time (memory stays n^2 at d = 256)."""
    r2 = np.zeros((A.shape[0], B.shape[0]))
    for c in range(A.shape[1]):
        diff = A[:, c, None] - B[None, :, c]
        r2 += diff * diff / ell[c] ** 2
    return r2


def log_marginal(X, Y, var, ell, bias, noise):
    return ArdPosterior(X, Y, var, ell, bias, noise, need_inv=False).log_marginal


class ArdPosterior:
    def __init__(self, X, Y, var, ell, bias, noise, need_inv=True):
        self.X = np.asarray(X, dtype=float)
        self.Y = np.asarray(Y, dtype=float).reshape(-1, 1)
        n, d = self.X.shape
        self.ell = np.broadcast_to(np.asarray(ell, dtype=float).reshape(-1), (d,)).copy()
        self.var, self.bias, self.noise = float(var), float(bias), float(noise)
        self.Krbf = self.var * np.exp(-0.5 * ard_r2(self.X, self.X, self.ell))
        Ky = self.Krbf + self.bias
        Ky[np.diag_indices(n)] += self.noise + JITTER
        self.L = sl.cholesky(Ky, lower=True)
        self.alpha = sl.cho_solve((self.L, True), self.Y)
        self.log_marginal = 0.5 * (-n * np.log(2 * np.pi) - 2. * np.sum(np.log(np.diag(self.L)))
                                   - float((self.Y.T @ self.alpha)[0, 0]))
        if need_inv:
            Linv = sl.solve_triangular(self.L, np.eye(n), lower=True)
            self.Kinv = Linv.T @ Linv

    def kern(self, A, B):
        """Prior covariance k(A, B)."""
        A, B = np.asarray(A, float).reshape(-1, self.X.shape[1]), np.asarray(B, float).reshape(-1, self.X.shape[1])
        return self.var * np.exp(-0.5 * ard_r2(A, B, self.ell)) + self.bias

    def log_marginal_grad(self):
        """d log Z / d (var, l_1 .. l_d, bias, noise) -- GPy's param_array order."""
        D = 0.5 * (self.alpha @ self.alpha.T - self.Kinv)
        E = D * self.Krbf
        g_ell = np.empty(self.X.shape[1])
        for c in range(self.X.shape[1]):
            diff = self.X[:, c, None] - self.X[None, :, c]
            g_ell[c] = np.sum(E * diff * diff) / self.ell[c] ** 3
        return np.concatenate([[np.sum(E) / self.var], g_ell, [np.sum(D), np.trace(D)]])

    def predict(self, x, noiseless=False):
        x = np.asarray(x, dtype=float).reshape(-1, self.X.shape[1])
        Kx = self.kern(self.X, x)                                                # (n, S)
        mu = Kx.T @ self.alpha
        v = np.clip((self.var + self.bias) - np.sum((self.Kinv @ Kx) * Kx, 0), 1e-15, np.inf)[:, None]
        return mu, v if noiseless else v + self.noise

    def predictive_gradients(self, x):
        x = np.asarray(x, dtype=float).reshape(-1, self.X.shape[1])
        Kx = self.kern(x, self.X)                                                # (S, n)
        Kr = Kx - self.bias
        dk = -Kr[:, :, None] * (x[:, None, :] - self.X[None, :, :]) / self.ell ** 2    # (S, n, d)
        return (np.einsum('snd,n->sd', dk, self.alpha[:, 0]), np.einsum('snd,sn->sd', dk, -2. * Kx @ self.Kinv))

    def cross_cov(self, P, x):
        """Posterior covariance (M, S) between the rows of P and of x."""
        return self.kern(P, x) - self.kern(P, self.X) @ self.Kinv @ self.kern(self.X, x)

    def lcb(self, x, beta):
        """(value (S, 1), gradient (S, d)) of mean - sqrt(beta var), noiseless variance (acquisition.py:256-301)."""
        mu, v = self.predict(x, noiseless=True)
        gm, gv = self.predictive_gradients(x)
        return mu - np.sqrt(beta * v), gm - 0.5 * gv * np.sqrt(beta / v)


# ---- the MAP objective of the hyper-parameter search, restated for 3 + d parameters ([GPy-upstream] paramz: Logexp
# transform theta = log(1 + exp(phi)), Gamma priors (a, b) with the transform's log-Jacobian on the parameters that carry
# one; elfi_amd/hyperopt.py's module text has the formulas)
def _logexp(phi):
    return np.where(phi > 36., phi, np.log1p(np.exp(np.minimum(phi, 36.))))


class MapObjective:
    """value(phi) and gradient(phi) of -(log Z + log prior) over phi for theta = (var, l_1 .. l_d, bias, noise); `priors`
    maps 'var' / 'ls' / 'bias' to Gamma (a, b), the one of 'ls' applying to every lengthscale."""

    def __init__(self, X, Y, priors):
        self.X, self.Y, self.priors = np.asarray(X, float), np.asarray(Y, float).reshape(-1, 1), priors
        d = self.X.shape[1]
        self.names = ('var',) + ('ls',) * d + ('bias', 'noise')

    def _both(self, phi):
        from scipy.special import gammaln
        theta = _logexp(np.asarray(phi, float))
        post = ArdPosterior(self.X, self.Y, theta[0], theta[1:-2], theta[-2], theta[-1])
        lp, dlp = 0.0, np.zeros(len(theta))
        for i, name in enumerate(self.names):
            if name in self.priors:
                a, b = self.priors[name]
                t = theta[i]
                lp += a * np.log(b) - gammaln(a) + (a - 1.) * np.log(t) - b * t + np.log(np.expm1(t)) - t
                dlp[i] = (a - 1.) / t - b + 1. / np.expm1(t)
        return -(post.log_marginal + lp), -(post.log_marginal_grad() + dlp) * -np.expm1(-theta)

    def value(self, phi):
        return self._both(phi)[0]

    def gradient(self, phi):
        return self._both(phi)[1]
