"""The search for the GP mean's minimiser (csrc/gp_min.hip, include/elfihip.h: elfihip_gp_minimize_mean) stated in NumPy.

SciPy's differential evolution with its defaults (best1bin, dither (0.5, 1), recombination 0.7, latin-hypercube start) in the
DEFERRED form, on Philox draws whose counter is a pure function of (generation, member, slot) -- nothing depends on how many
out-of-box coordinates were redrawn -- over a NumPy GP mean with the device's arithmetic:

    r2 = (|x|^2 + |X_i|^2) - 2 x.X_i  clipped at 0,   k = s_f exp(r2 (-1 / 2 l^2)),   mu = sum_i (k + s_b) alpha_i

(the sum in NumPy's order: the device's fixed order differs from it in the last bits only).  The polish is SciPy's L-BFGS-B
with its defaults on the mean and its analytic gradient -- the algorithm the library's own L-BFGS-B (csrc/lbfgsb.hpp)
follows -- from the best member, accepted only if it lowers the energy.
"""
import numpy as np

from philox_ref import uniform53_first

CR = 0.7
STREAM = 0x44454D494E000000   # elfi_amd.priors.GP_MINIMIZE_STREAM_BASE


def n_slots(d):
    return 2 * d + 4


def counter(g, i, slot, d):
    """The 64-bit Philox counter of draw (generation, member, slot): low word i (2 d + 4) + slot, high word g."""
    return (np.asarray(g, dtype=np.uint64) << np.uint64(32)) | \
        (np.asarray(i, dtype=np.uint64) * np.uint64(n_slots(d)) + np.asarray(slot, dtype=np.uint64))


def draw(seed, stream, g, i, slot, d):
    return uniform53_first(seed, stream, counter(g, i, slot, d))


class GPMean:
    """mu(x) from the evidence X (n, d), alpha (n,) and the hyper-parameters, with the device's terms."""

    def __init__(self, X, alpha, var, ls, bias):
        self.X = np.asarray(X, dtype=np.float64)
        self.alpha = np.asarray(alpha, dtype=np.float64).reshape(-1)
        self.var, self.ls, self.bias = float(var), float(ls), float(bias)
        self.X2 = np.zeros(self.X.shape[0])
        for c in range(self.X.shape[1]):      # ascending order of the dimension, as the library sums |x|^2
            self.X2 = self.X2 + self.X[:, c] * self.X[:, c]

    def kernel(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.X.shape[1])
        x2 = np.zeros(x.shape[0])
        for c in range(x.shape[1]):
            x2 = x2 + x[:, c] * x[:, c]
        r2 = np.maximum((x2[:, None] + self.X2[None, :]) + (-2.0 * (x @ self.X.T)), 0.0)
        return self.var * np.exp(r2 * (-0.5 / (self.ls * self.ls)))

    def __call__(self, x):
        return (self.kernel(x) + self.bias) @ self.alpha

    def gradient(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.X.shape[1])
        k = self.kernel(x)
        diff = x[:, None, :] - self.X[None, :, :]
        return np.einsum('sn,snd->sd', -(k / self.ls ** 2) * self.alpha[None, :], diff)


def scale(p, lo, hi):
    """Unit coordinates -> the box (SciPy's _scale_parameters)."""
    return 0.5 * (lo + hi) + (p - 0.5) * np.abs(hi - lo)


def start_population(d, NP, seed, stream=STREAM):
    """Latin hypercube: member i, dimension j = (perm_j(i) + u_ij) / NP with perm_j the stable argsort of NP uniforms."""
    i, j = np.arange(NP)[:, None], np.arange(d)[None, :]
    order = draw(seed, stream, 0, i, 3 + j, d)
    perm = np.argsort(order, axis=0, kind='stable')
    return (perm.astype(np.float64) + draw(seed, stream, 0, i, 3 + d + j, d)) / float(NP)


def best_member(E):
    return int(np.argmin(E))     # the first of equal minima


def trials(pop, E, g, seed, stream=STREAM):
    """The NP trial vectors of generation g >= 1 from the population of generation g - 1."""
    NP, d = pop.shape
    i = np.arange(NP)
    F = 0.5 + 0.5 * float(draw(seed, stream, g, 0, 3 + 2 * d, d))
    r0 = np.minimum((draw(seed, stream, g, i, 0, d) * (NP - 1)).astype(np.int64), NP - 2)
    r0 = r0 + (r0 >= i)
    r1 = np.minimum((draw(seed, stream, g, i, 1, d) * (NP - 2)).astype(np.int64), NP - 3)
    r1 = r1 + (r1 >= np.minimum(i, r0))
    r1 = r1 + (r1 >= np.maximum(i, r0))
    fill = np.minimum((draw(seed, stream, g, i, 2, d) * d).astype(np.int64), d - 1)
    j = np.arange(d)[None, :]
    cross = (draw(seed, stream, g, i[:, None], 3 + j, d) < CR) | (j == fill[:, None])
    mutant = pop[best_member(E)][None, :] + F * (pop[r0] - pop[r1])
    trial = np.where(cross, mutant, pop)
    out = (trial < 0.0) | (trial > 1.0)
    return np.where(out, draw(seed, stream, g, i[:, None], 3 + d + j, d), trial), dict(F=F, r0=r0, r1=r1, fill=fill)


def converged(E, tol):
    return bool(np.std(E) <= tol * abs(np.mean(E)))


def minimize(mean, lo, hi, seed=0, stream=STREAM, popsize=15, maxiter=1000, tol=0.01, polish=True, trace=None):
    """-> dict(x, f, pop, energies, generations, evaluations, converged, polish_accepted).  `trace`, a list, receives per
    generation the smallest |E_trial - E_member| (how close the closest accept comparison was).  `polish` needs a `mean`
    with a `gradient` method."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    d = lo.shape[0]
    NP = max(5, popsize * d)
    pop = start_population(d, NP, seed, stream)
    E = mean(scale(pop, lo, hi))
    if not np.all(np.isfinite(E)):
        raise FloatingPointError('the mean is not finite at a start point')
    g, done = 0, False
    while g < maxiter:
        g += 1
        T, _ = trials(pop, E, g, seed, stream)
        Et = mean(scale(T, lo, hi))
        if not np.all(np.isfinite(Et)):
            raise FloatingPointError('the mean is not finite at a trial point')
        if trace is not None:
            trace.append(float(np.min(np.abs(Et - E))))
        take = Et <= E
        pop, E = np.where(take[:, None], T, pop), np.where(take, Et, E)
        if converged(E, tol):
            done = True
            break
    b = best_member(E)
    x, f, nfev, accepted = np.clip(scale(pop[b], lo, hi), lo, hi), float(E[b]), NP * (g + 1), False
    if polish:
        from scipy.optimize import minimize as scipy_minimize
        res = scipy_minimize(lambda v: (float(mean(v)[0]), mean.gradient(v)[0]), x, jac=True, method='L-BFGS-B',
                             bounds=list(zip(lo, hi)))
        fp = float(mean(res.x)[0])
        nfev += res.nfev + 1
        if fp < f:
            x, f, accepted = res.x, fp, True
    return dict(x=x, f=f, pop=pop, energies=E, generations=g, evaluations=nfev, converged=done, polish_accepted=accepted)
