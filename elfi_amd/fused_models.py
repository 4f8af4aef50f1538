"""ELFI's example models with the whole simulation on the GPU: same priors, same node names, same inference calls.

    m = elfi_amd.fused_models.ma2_model(n_obs=100, seed_obs=4)        # elfi.examples.ma2.get_model(...)
    m = elfi_amd.fused_models.gauss_model(n_obs=50, seed_obs=4)       # elfi.examples.gauss.get_model(...)
    m = elfi_amd.fused_models.arch_model(n_obs=100, seed_obs=4)       # elfi.examples.arch.get_model(...)
    m = elfi_amd.fused_models.mg1_model(n_obs=50, seed_obs=4)         # elfi.examples.mg1.get_model(...)
    m = elfi_amd.fused_models.lorenz_model(seed_obs=4)                # elfi.examples.lorenz.get_model(...)
    m = elfi_amd.fused_models.gnk_model(n_obs=50, seed=4)             # elfi.examples.gnk.get_model(...)
    m = elfi_amd.fused_models.bignk_model(n_obs=150, seed=4)          # elfi.examples.bignk.get_model(...)
    m = elfi_amd.fused_models.ricker_model(n_obs=50, seed_obs=4)      # elfi.examples.ricker.get_model(...)
    m = elfi_amd.fused_models.lotka_volterra_model(seed_obs=4)        # elfi.examples.lotka_volterra.get_model(...)
    m = elfi_amd.fused_models.daycare_model(seed_obs=4)               # elfi.examples.daycare.get_model(...)
    m = elfi_amd.fused_models.toad_model(seed_obs=4)                  # elfi.examples.toad.get_model(...)
    m = elfi_amd.fused_models.sv_model(n_obs=50, seed_obs=4)          # elfi.examples.stochastic_volatility_model.get_model(...)
    m = elfi_amd.fused_models.bdm_model()                             # elfi.examples.bdm.get_model(...), no executable
    m = elfi_amd.fused_models.ar1_model(n_obs=200, seed_obs=4)        # elfi.examples.ar1.get_model(...)
    elfi_amd.HipRejection(m['d'], batch_size=10**6, seed=1).sample(1000, n_sim=10**8)

The reference's Simulator node draws the series on the host (MA2: random_state.randn(batch, n_obs + 2),
elfi/examples/ma2.py:35; gauss: ss.norm.rvs(size=(batch, n_obs)), elfi/examples/gauss.py:31-33) -- 0.8 KB per
simulation -- and the Summary nodes reduce it again.  Here the Simulator node's operation IS the fused device kernel
(csrc/summaries.hip ma2 / csrc/gauss.hip): the draws (Philox4x32-10, keyed by a seed taken from the node's own
random_state, so ELFI's batch seeding decides them: elfi/loader.py:164-169), the simulator arithmetic and both summaries
in one pass; the series never exists in memory.  What the node returns is the (batch, 2) array of summaries; the
Summary nodes pick their column and the Distance node is elfi.Distance over elfi_amd.HipDistance.  The observed data are
generated exactly as the reference's get_model does (its own simulator on the host with RandomState(seed_obs)) and
reduced to the observed summaries once, at model construction.

arch_model / mg1_model are the reference's time-series examples (elfi/examples/arch.py, mg1.py) built the same way on
csrc/series.hip: each simulation has a serial recurrence (a chain of dependent square roots; two running sums and a
maximum), which one lane walks while the draws and the reductions keep the wavefront busy.  Their Simulator node returns
all summaries of a simulation -- ARCH: the (batch, 2 + L + L (L - 1) / 2) columns MU, VAR, AC_1 .., PW_1_2 ..; M/G/1:
(batch, n_obs + n_quantiles) = [log inter-departure times | quantiles] -- and the Summary nodes slice columns; M/G/1's
log_identity is what HipBSL / syn_loglik take.  On given draws series, summaries and quantiles are the reference's bit
for bit, the logarithms within 4 ulp (tests/test_series_models_gpu.py).

lorenz_model is the stochastic Lorenz-96 forecast example (elfi/examples/lorenz.py: 40 coupled variables, 160 rows, a
fourth-order Runge-Kutta step and an AR(1) forcing per row, six summaries) on csrc/lorenz.hip: a simulation is one
wavefront, a variable one lane; its Simulator node returns the (batch, 6) columns Mean, Var, Autocov, Cov, CrosscovPrev,
CrosscovNext.  On given draws series and summaries are the reference's bit for bit (tests/test_lorenz_gpu.py).

gnk_model / bignk_model are the g-and-k quantile-distribution examples (elfi/examples/gnk.py, bignk.py) on csrc/gnk.hip.
Nothing in them is a recurrence: the wavefront's lanes take single elements for the exp and pow of the quantile function
and whole columns for the sort that the octiles need.  The Simulator node returns the (batch, m) rows of the ONE summary
the model was built with (gnk: 'order', the reference's default; bignk: 'robust'), the Summary node ss_<summary> gives them
the reference's (batch, m, 1) shape, and d is an elfi.Discrepancy that flattens them for HipDistance('euclidean') -- the
reference's euclidean_multiss up to the order of its sum.  The series goes through the device's exp and pow: within a few
eps (|A| + |y - A|) of the reference's on given draws, and every summary NumPy's bit for bit on that series
(tests/test_gnk_gpu.py).  The bivariate model's correlated normals are z0 = e0, z1 = rho e0 + sqrt(1 - rho^2) e1 of the
device generator: the distribution of the reference's multivariate_normal.rvs draws, not their bits.

ricker_model is the Ricker example (elfi/examples/ricker.py: a chaotic stock recurrence observed through a Poisson count;
the deterministic variant without noise and observation layer) on csrc/series.hip, built like arch_model: a lane walks the
stock of its simulation, then the wavefront draws the tile's Poisson counts element by element with the library's
counter-based sampler (csrc/poisson.hpp: inversion below an intensity of 10, transformed rejection from there on).  Its
Simulator node returns the (batch, 3) columns Mean, Var, #0; d is an elfi.Discrepancy over the reference's chi_squared
stated in NumPy (deterministic: elfi.Distance over HipDistance('euclidean') on Mean).  Each step of the stock is within 4
ulp of NumPy's on the same previous stock, the counts are the NumPy statement's of the sampler and the summaries NumPy's bit
for bit on the device's counts (tests/test_ricker_gpu.py).  An overflowed stock is observed as NaN, where the reference
raises ValueError for the whole batch.

lotka_volterra_model is the stochastic predator-prey example (elfi/examples/lotka_volterra.py: a Markov jump process
simulated by Gillespie's direct method, whose number of events per simulation varies over three orders of magnitude under
the priors) on csrc/gillespie.hip: one lane per simulation in persistent wavefronts that take the next simulation from a
counter as soon as theirs ends, observations emitted as the events pass their times, then the nine summaries.  Its
Simulator node LV returns the (batch, 9) summaries, the Summary nodes pick their column, d is elfi.Distance over
HipDistance('euclidean').  Observations, event counts and final times are the NumPy statement's bit for bit on given draws;
the summaries are NumPy's bit for bit except the two log-variances (within 4 ulp, the device's log)
(tests/test_lotka_volterra_gpu.py).  A simulation is cut off after max_events events (default 2^20) with NaN summaries, where
the reference runs on without bound.

daycare_model is the pneumococcal day-care-centre transmission example (elfi/examples/daycare.py: the model BOLFI was
introduced on; a Markov jump process over the carriage of 33 strains by the 53 individuals of each of 29 centres) on
csrc/daycare.hip: one wavefront per (simulation, centre) pair, taken from a counter, with the factorised hazard.  Its Simulator
node DCC returns the (batch, 4, n_dcc) summaries of every centre, the Summary nodes Shannon, n_strains, prevalence and multi pick
their (batch, n_dcc) slice, d is an elfi.Discrepancy over elfi_amd.daycare_distance (the example's sorted L1 distance, on the
device) and logd its logarithm: the node BOLFI is meant to model.  Every centre stops at its own first event at or past
time_end; the reference keeps all of a batch jumping until the slowest has passed it, so it is reproduced exactly -- final
states and event counts on given draws -- per centre (tests/test_daycare.py, tests/test_daycare_gpu.py).

toad_model is Marchand's toad movement example (elfi/examples/toad.py: 66 toads over 63 days, alpha-stable foraging steps
and returns to earlier refuges; An, Nott and Drovandi's 48 summaries, the standard BSL test problem) on csrc/toad.hip: one
workgroup per simulation keeps the positions in LDS, every lane makes steps (the library's stable-law sampler,
csrc/stable.hpp), a lane per toad walks its chain, and per lag the workgroup sorts the displacements of the toads that did not
return (csrc/wg_sort.hpp).  Its Simulator node toad returns the (batch, 48) summaries, the Summary nodes S1, S2, S4, S8 slice
their 12 columns -- what HipBSL / syn_loglik take.  On given steps the positions are NumPy's bit for bit, on the positions the
counts and medians are, the log quantile differences within 4 ulp (tests/test_toad.py, tests/test_toad_gpu.py).

sv_model is the alpha-stable stochastic-volatility example (elfi/examples/stochastic_volatility_model.py: AR(1)
log-volatilities under skewed alpha-stable shocks; the test problem of Priddle and Drovandi's semiparametric synthetic
likelihood) on csrc/sv.hip: one workgroup per simulation (one wavefront up to 1024 observations), every lane makes the draws
and the shock of its cells (the general stable sampler of csrc/stable.hpp, S0 parameterisation), one lane walks the chain,
and the workgroup sorts the returns for the two quantile summaries.  Its Simulator node a_svm returns (batch, n_obs + 2): the
returns, kurt, skew; the Summary nodes returns, kurt and skew slice its columns.  On given normals the chain is NumPy's bit
for bit, on the returns the summaries are; each shock is within twice its first-order bound of SciPy's expression in NumPy
(tests/test_sv.py, tests/test_sv_gpu.py).  An invalid parameter row is NaN, where SciPy raises for the whole batch.

bdm_model is the birth-death-mutation example (elfi/examples/bdm.py: the model of Lintusaari et al. 2017, the reference's
showcase for elfi.tools.external_operation -- a text file, a `bdm` executable compiled by hand and two deleted files per batch)
on csrc/bdm.hip: a jump chain of a few dozen to a thousand events, one wavefront per simulation.  Its Simulator node BDM
returns the (batch, N) clusters as int16, T1 is the reference's own function on them, d is elfi.Distance over
HipDistance('minkowski', p=1).  On the replayed uniforms of the reference binary the clusters are its clusters
(tests/test_bdm.py, tests/test_bdm_gpu.py).  Two differences: the parameters are not rounded to 4 decimals on the way (the
reference's text file does), and with seed_obs given or N != 20 the observed data are one DEVICE simulation where the
reference calls its binary.

ar1_model is the AR(1) example (elfi/examples/ar1.py) on csrc/series.hip, a lane per simulation like arch_model; its
Simulator node AR1 returns the (batch, n_obs) series, bit for bit the reference's on given noise (tests/test_ar1_gpu.py), and d
is elfi.Distance over HipDistance('euclidean') on it.

The draws are the device generator's, not MT19937's: a run of this model is a different (equally valid) random
realisation than a run of elfi.examples.*.get_model with the same seed; the arithmetic on given draws is bit-identical
to the reference's (tests/test_summaries_gpu.py, tests/test_gauss_gpu.py).
"""
import sys
from functools import partial
from itertools import combinations

import numpy as np

from .distance import HipDistance, randn_rows
from .priors import SIMULATOR_STREAM_BASE
from .summaries import LORENZ_NAMES, arch_summaries, gauss_distance, lorenz_summaries, ma2_draw_distance, mg1_summaries
from .summaries import GNK_SUMMARIES, bignk_summaries, gnk_summaries
from .summaries import RICKER_NAMES, ricker_summaries
from .summaries import LV_NAMES, lotka_volterra_summaries
from .summaries import DAYCARE_NAMES, daycare_distance, daycare_summaries
from .summaries import TOAD_LAGS, toad_summaries
from .summaries import sv_summaries
from .summaries import scratch_assay_summaries
from .summaries import ar1_series, bdm_clusters


def _elfi():
    mod = sys.modules.get('elfi')
    if mod is None:
        raise ImportError('the fused models are built from the running program\'s ELFI: `import elfi` first')
    return mod


def _seed_of(random_state):
    rs = random_state or np.random
    return int(rs.randint(0, 2 ** 31 - 1))


def ma2_summaries(t1, t2, observed_summaries=(0.0, 0.0), n_obs=100, batch_size=1, random_state=None):
    """Simulator operation: (batch, 2) = [autocov(x, 1), autocov(x, 2)] of MA2 series drawn and reduced on the device."""
    S1, S2, _ = ma2_draw_distance(t1, t2, observed_summaries, n_obs=n_obs, seed=_seed_of(random_state),
                                  stream=SIMULATOR_STREAM_BASE)
    return np.column_stack((S1, S2))


def gauss_summaries(mu, sigma, observed_summaries=(0.0, 0.0), n_obs=50, batch_size=1, random_state=None):
    """Simulator operation: (batch, 2) = [mean(y), var(y)] of Gaussian samples drawn and reduced on the device."""
    S1, S2, _ = gauss_distance(mu, sigma, observed_summaries, n_obs=n_obs, seed=_seed_of(random_state),
                               stream=SIMULATOR_STREAM_BASE)
    return np.column_stack((S1, S2))


def first_column(y):
    return np.asarray(y)[:, 0]


def second_column(y):
    return np.asarray(y)[:, 1]


def ma2_model(n_obs=100, true_params=None, seed_obs=None, device_priors=True):
    """elfi.examples.ma2.get_model(n_obs, true_params, seed_obs) with the simulation on the device; nodes t1, t2, MA2,
    S1, S2, d.  device_priors: the two Prior nodes draw on the device as well (elfi_amd.priors: same distributions, the
    library's generator; False keeps the reference's CustomPrior1 / CustomPrior2 and their SciPy draws)."""
    elfi = _elfi()
    from elfi.examples import ma2
    if true_params is None:
        true_params = [.6, .2]
    y = ma2.MA2(*true_params, n_obs=n_obs, random_state=np.random.RandomState(seed_obs))
    obs = np.array([[ma2.autocov(y)[0], ma2.autocov(y, 2)[0]]])
    m = elfi.ElfiModel()
    from . import priors
    elfi.Prior(priors.MA2Prior1 if device_priors else ma2.CustomPrior1, 2, model=m, name='t1')
    elfi.Prior(priors.MA2Prior2 if device_priors else ma2.CustomPrior2, m['t1'], 1, name='t2')
    elfi.Simulator(partial(ma2_summaries, observed_summaries=tuple(obs[0]), n_obs=n_obs), m['t1'], m['t2'], observed=obs,
                   name='MA2')
    elfi.Summary(first_column, m['MA2'], name='S1')
    elfi.Summary(second_column, m['MA2'], name='S2')
    elfi.Distance(HipDistance('euclidean'), m['S1'], m['S2'], name='d')
    return m


def gauss_model(n_obs=50, true_params=None, seed_obs=None, device_priors=True):
    """elfi.examples.gauss.get_model(n_obs, true_params, seed_obs) (1-D mean and standard deviation) with the simulation
    on the device; nodes mu, sigma, gauss, ss_mean, ss_var, d.  device_priors: the uniform prior of mu draws on the device
    (sigma's truncated normal stays SciPy's)."""
    elfi = _elfi()
    from elfi.examples import gauss
    if true_params is None:
        true_params = [4, .4]
    y = gauss.gauss(*true_params, n_obs=n_obs, random_state=np.random.RandomState(seed_obs))
    obs = np.array([[gauss.ss_mean(y)[0], gauss.ss_var(y)[0]]])
    m = elfi.new_model()
    eps_prior = 5
    from . import priors
    mu = elfi.Prior(priors.uniform if device_priors else 'uniform', true_params[0] - eps_prior, 2 * eps_prior, model=m,
                    name='mu')
    sigma = elfi.Prior('truncnorm', np.amax([.01, true_params[1] - eps_prior]), 2 * eps_prior, model=m, name='sigma')
    elfi.Simulator(partial(gauss_summaries, observed_summaries=tuple(obs[0]), n_obs=n_obs), mu, sigma, observed=obs,
                   name='gauss')
    elfi.Summary(first_column, m['gauss'], name='ss_mean')
    elfi.Summary(second_column, m['gauss'], name='ss_var')
    elfi.Distance(HipDistance('euclidean'), m['ss_mean'], m['ss_var'], name='d')
    return m


def column(y, j=0):
    return np.asarray(y)[:, j]


def columns(y, start=0, stop=None):
    return np.asarray(y)[:, start:stop]


def _per_simulation(batch_size, *params):
    """Parameters fixed to one value (model.generate(..., with_values=...)) are repeated over the batch."""
    params = [np.asarray(p, dtype=np.float64).reshape(-1) for p in params]
    n = max([int(batch_size)] + [p.shape[0] for p in params])
    return [np.repeat(p, n) if p.shape[0] == 1 and n > 1 else p for p in params]


def arch_summary_rows(t1, t2, n_obs=100, n_lags=5, batch_size=1, random_state=None):
    """Simulator operation: (batch, 2 + L + L (L - 1) / 2) summaries MU, VAR, AC_1 .., PW_1_2 .. of ARCH(1) series drawn,
    run and reduced on the device."""
    t1, t2 = _per_simulation(batch_size, t1, t2)
    return arch_summaries(t1, t2, n_obs=n_obs, n_lags=n_lags, seed=_seed_of(random_state), stream=SIMULATOR_STREAM_BASE)


def arch_names(n_lags=5):
    lags = range(1, n_lags + 1)
    return ['MU', 'VAR'] + ['AC_%d' % i for i in lags] + ['PW_%d_%d' % ij for ij in combinations(lags, 2)]


def arch_model(n_obs=100, true_params=None, seed_obs=None, n_lags=5, device_priors=True):
    """elfi.examples.arch.get_model(n_obs, true_params, seed_obs, n_lags) with the simulation on the device; nodes t1,
    t2, Y, MU, VAR, AC_i, PW_i_j, d.  The node Y returns the (batch, m) summaries, the Summary nodes pick their column.
    device_priors: the two uniform priors draw on the device as well (elfi_amd.priors.uniform; False: SciPy's)."""
    elfi = _elfi()
    from elfi.examples import arch
    if true_params is None:
        true_params = [0.3, 0.7]
    y = arch.arch(*true_params, n_obs=n_obs, random_state=np.random.RandomState(seed_obs))
    lags = range(1, n_lags + 1)
    obs = np.column_stack([arch.sample_mean(y), arch.sample_variance(y)] + [arch.autocorr(y, i) for i in lags] +
                          [arch.pairwise_autocorr(y, i, j) for i, j in combinations(lags, 2)])
    m = elfi.ElfiModel()
    from . import priors
    uniform = priors.uniform if device_priors else 'uniform'
    elfi.Prior(uniform, -1, 2, model=m, name='t1')
    elfi.Prior(uniform, 0, 1, model=m, name='t2')
    elfi.Simulator(partial(arch_summary_rows, n_obs=n_obs, n_lags=n_lags), m['t1'], m['t2'], observed=obs, name='Y')
    ss = [elfi.Summary(partial(column, j=k), m['Y'], name=name) for k, name in enumerate(arch_names(n_lags))]
    elfi.Distance(HipDistance('euclidean'), *ss, name='d')
    return m


def mg1_summary_rows(t1, t2, t3, n_obs=50, q=None, batch_size=1, random_state=None):
    """Simulator operation: (batch, n_obs + nq) = [log inter-departure times | quantiles] of M/G/1 series drawn, run,
    sorted and reduced on the device."""
    t1, t2, t3 = _per_simulation(batch_size, t1, t2, t3)
    logy, quant = mg1_summaries(t1, t2, t3, n_obs=n_obs, q=q, seed=_seed_of(random_state), stream=SIMULATOR_STREAM_BASE)
    return np.hstack((logy, quant))


def mg1_model(n_obs=50, true_params=None, seed_obs=None, n_quantiles=10, device_priors=True):
    """elfi.examples.mg1.get_model(n_obs, true_params, seed_obs, n_quantiles) with the simulation on the device; nodes t1,
    t2, t3, MG1, log_identity, quantiles, d.  The node MG1 returns [log y | quantiles] per simulation, the two Summary
    nodes slice it.  device_priors: t1 and t3 draw on the device (t2, whose location is the node t1, stays SciPy's)."""
    elfi = _elfi()
    from elfi.examples import mg1
    if true_params is None:
        true_params = [1., 5., 0.2]
    y = mg1.MG1(*true_params, n_obs=n_obs, random_state=np.random.RandomState(seed_obs))
    q = np.linspace(0, 1, n_quantiles)
    obs = np.hstack((mg1.log_identity(y), mg1.quantiles(y, q)))
    m = elfi.ElfiModel()
    from . import priors
    uniform = priors.uniform if device_priors else 'uniform'
    elfi.Prior(uniform, 0, 10, model=m, name='t1')
    elfi.Prior('uniform', m['t1'], 10, model=m, name='t2')   # t2 - t1 ~ U(0, 10)
    elfi.Prior(uniform, 0, 0.5, model=m, name='t3')
    elfi.Simulator(partial(mg1_summary_rows, n_obs=n_obs, q=q), m['t1'], m['t2'], m['t3'], observed=obs, name='MG1')
    elfi.Summary(partial(columns, stop=n_obs), m['MG1'], name='log_identity')
    elfi.Summary(partial(columns, start=n_obs), m['MG1'], name='quantiles')
    elfi.Distance(HipDistance('euclidean', w=(1 / 100) ** q), m['quantiles'], name='d')
    return m


class _InitialState(np.ndarray):
    """An initial state the reference's simulator accepts: forecast_lorenz tests `if not initial_state` (lorenz.py:128),
    which an array of more than one element refuses to answer."""

    def __bool__(self):
        return True


def lorenz_summary_rows(theta1, theta2, initial_state=None, f=10., phi=0.984, n_obs=40, n_timestep=160, total_duration=4,
                        batch_size=1, random_state=None):
    """Simulator operation: (batch, 6) summaries Mean, Var, Autocov, Cov, CrosscovPrev, CrosscovNext of stochastic Lorenz-96
    series drawn, integrated and reduced on the device."""
    theta1, theta2 = _per_simulation(batch_size, theta1, theta2)
    return lorenz_summaries(theta1, theta2, initial_state, f=f, phi=phi, n_obs=n_obs, n_timestep=n_timestep,
                            total_duration=total_duration, seed=_seed_of(random_state), stream=SIMULATOR_STREAM_BASE)


def lorenz_model(true_params=None, seed_obs=None, initial_state=None, n_obs=40, f=10., phi=0.984, total_duration=4,
                 device_priors=True):
    """elfi.examples.lorenz.get_model(true_params, seed_obs, initial_state, n_obs, f, phi, total_duration) with the
    simulation on the device; nodes theta1, theta2, Lorenz, Mean, Var, Autocov, Cov, CrosscovPrev, CrosscovNext, d.  The
    node Lorenz returns the (batch, 6) summaries, the Summary nodes pick their column.  The observed series is the
    reference's own forecast_lorenz with RandomState(seed_obs), reduced once with its summary functions; its default
    initial state (n_obs = 40) is asked of that simulator, whose row 0 it is.  device_priors: the two uniform priors draw
    on the device as well (elfi_amd.priors.uniform; False: SciPy's)."""
    elfi = _elfi()
    from elfi.examples import lorenz
    if true_params is None:
        true_params = [2.0, 0.1]
    if initial_state is None:
        y0 = np.array(lorenz.forecast_lorenz(0, 0, n_obs=n_obs, n_timestep=1, batch_size=1)[0, 0], dtype=np.float64)
        given = None
    else:
        y0 = np.array(initial_state, dtype=np.float64).reshape(-1)
        if y0.shape[0] != n_obs:
            raise ValueError('initial_state must hold the n_obs = %d initial values' % n_obs)
        given = y0.reshape(1, n_obs).view(_InitialState)
    y = lorenz.forecast_lorenz(*true_params, f=f, phi=phi, n_obs=n_obs, initial_state=given, total_duration=total_duration,
                               random_state=np.random.RandomState(seed_obs))
    y = np.asarray(y)
    n_timestep = y.shape[1]
    obs = np.column_stack([lorenz.mean(y), lorenz.var(y), lorenz.autocov(y), lorenz.cov(y), lorenz.xcov(y, True),
                           lorenz.xcov(y, False)])
    m = elfi.ElfiModel()
    from . import priors
    uniform = priors.uniform if device_priors else 'uniform'
    elfi.Prior(uniform, 0.5, 3., model=m, name='theta1')
    elfi.Prior(uniform, 0, 0.3, model=m, name='theta2')
    elfi.Simulator(partial(lorenz_summary_rows, initial_state=y0, f=f, phi=phi, n_obs=n_obs, n_timestep=n_timestep,
                           total_duration=total_duration), m['theta1'], m['theta2'], observed=obs, name='Lorenz')
    ss = [elfi.Summary(partial(column, j=k), m['Lorenz'], name=name) for k, name in enumerate(LORENZ_NAMES)]
    elfi.Distance(HipDistance('euclidean'), *ss, name='d')
    return m


def rows_as_points(y):
    """Summary operation of the g-and-k models: the (batch, m) rows in the reference's (batch, m, 1) shape."""
    return np.asarray(y)[:, :, np.newaxis]


def euclidean_rows(*simulated, observed):
    """Discrepancy operation of the g-and-k models (the reference's euclidean_multiss, gnk.py:115-142, on one summary of
    shape (batch, m, 1)): flattened and handed to HipDistance('euclidean')."""
    sim = np.asarray(simulated[0])
    return HipDistance('euclidean')(sim.reshape(sim.shape[0], -1), np.asarray(observed[0]).reshape(1, -1))


def gnk_summary_rows(*params, dim=1, c=0.8, n_obs=50, summary='order', batch_size=1, random_state=None):
    """Simulator operation: the (batch, m) rows of one summary of g-and-k series (dim = 1) or bivariate g-and-k series
    (dim = 2) drawn, transformed, sorted and read on the device."""
    params = _per_simulation(batch_size, *params)
    fn = gnk_summaries if dim == 1 else bignk_summaries
    return fn(*params, c=c, n_obs=n_obs, summary=summary, seed=_seed_of(random_state), stream=SIMULATOR_STREAM_BASE)


def _observed_rows(module, y_obs, summary):
    """The observed series through the reference's own summary function, as the (1, m) row the Simulator node holds."""
    if summary == 'sorted':      # not a reference summary: what ss_order was meant to be
        s = np.sort(np.asarray(y_obs), axis=1)
    else:
        s = getattr(module, 'ss_' + summary)(y_obs)
    return np.asarray(s, dtype=np.float64).reshape(1, -1)


def gnk_model(n_obs=50, true_params=None, seed=None, summary='order', device_priors=True):
    """elfi.examples.gnk.get_model(n_obs, true_params, seed) with the simulation on the device; nodes A, B, g, k, GNK,
    ss_<summary>, d.  summary: 'order' (the reference's default: the series as it is), 'octile', 'robust' or 'sorted'
    (true order statistics; not a reference summary).  The node GNK returns the (batch, m) rows of that summary, the
    Summary node gives them the reference's (batch, m, 1) shape and d is an elfi.Discrepancy over HipDistance('euclidean').
    The observed series is the reference's own GNK with RandomState(seed), reduced by its own summary function.
    device_priors: the four uniform priors draw on the device as well (elfi_amd.priors.uniform; False: SciPy's)."""
    elfi = _elfi()
    from elfi.examples import gnk
    if summary not in GNK_SUMMARIES:
        raise ValueError('summary must be one of %s' % (GNK_SUMMARIES,))
    if true_params is None:
        true_params = [3, 1, 2, .5]
    m = elfi.new_model()
    from . import priors
    uniform = priors.uniform if device_priors else 'uniform'
    nodes = [elfi.Prior(uniform, 0, 10, model=m, name=name) for name in ('A', 'B', 'g', 'k')]
    y_obs = gnk.GNK(*true_params, n_obs=n_obs, random_state=np.random.RandomState(seed))
    elfi.Simulator(partial(gnk_summary_rows, dim=1, n_obs=n_obs, summary=summary), *nodes,
                   observed=_observed_rows(gnk, y_obs, summary), name='GNK')
    ss = elfi.Summary(rows_as_points, m['GNK'], name='ss_' + summary)
    elfi.Discrepancy(euclidean_rows, ss, name='d')
    return m


def bignk_model(n_obs=150, true_params=None, seed=None, summary='robust', device_priors=True):
    """elfi.examples.bignk.get_model(n_obs, true_params, seed) with the simulation on the device; nodes a1, a2, b1, b2,
    g1, g2, k1, k2, rho, BiGNK, ss_<summary>, d.  summary: 'robust' (the reference's default), 'octile' or 'sorted'; 'order'
    is refused here, because the reference's ss_order would sort each (y0, y1) pair, which is no summary of either
    dimension.  Built as gnk_model is; the observed series is the reference's own BiGNK with RandomState(seed).  The device's
    correlated normals have the distribution of the reference's, not their bits."""
    elfi = _elfi()
    from elfi.examples import bignk, gnk
    if summary not in GNK_SUMMARIES or summary == 'order':
        raise ValueError("summary must be one of 'robust', 'octile', 'sorted'")
    if true_params is None:
        true_params = [3, 4, 1, 0.5, 1, 2, .5, .4, 0.6]
    m = elfi.new_model()
    from . import priors
    uniform = priors.uniform if device_priors else 'uniform'
    eps = np.finfo(float).eps
    ranges = [('a1', 0, 5), ('a2', 0, 5), ('b1', 0, 5), ('b2', 0, 5), ('g1', -5, 10), ('g2', -5, 10), ('k1', -.5, 5.5),
              ('k2', -.5, 5.5), ('rho', -1 + eps, 2 - 2 * eps)]
    nodes = [elfi.Prior(uniform, loc, scale, model=m, name=name) for name, loc, scale in ranges]
    y_obs = bignk.BiGNK(*true_params, n_obs=n_obs, random_state=np.random.RandomState(seed))
    elfi.Simulator(partial(gnk_summary_rows, dim=2, n_obs=n_obs, summary=summary), *nodes,
                   observed=_observed_rows(gnk, y_obs, summary), name='BiGNK')
    ss = elfi.Summary(rows_as_points, m['BiGNK'], name='ss_' + summary)
    elfi.Discrepancy(euclidean_rows, ss, name='d')
    return m


def ricker_summary_rows(log_rate, std=None, scale=None, stock_init=1., n_obs=50, batch_size=1, random_state=None):
    """Simulator operation: (batch, 3) summaries Mean, Var, #0 of Ricker series drawn, run, observed and reduced on the
    device (std = scale = None: the deterministic model)."""
    if std is None:
        log_rate, = _per_simulation(batch_size, log_rate)
    else:
        log_rate, std, scale = _per_simulation(batch_size, log_rate, std, scale)
    return ricker_summaries(log_rate, std, scale, stock_init=stock_init, n_obs=n_obs, seed=_seed_of(random_state),
                            stream=SIMULATOR_STREAM_BASE)


def chi_squared(*simulated, observed):
    """Discrepancy operation of the Ricker model: the reference's chi_squared (ricker.py:147-161)."""
    simulated = np.column_stack(simulated)
    observed = np.column_stack(observed)
    with np.errstate(all='ignore'):
        return np.sum((simulated - observed) ** 2. / observed, axis=1)


def ricker_model(n_obs=50, true_params=None, seed_obs=None, stochastic=True, device_priors=True):
    """elfi.examples.ricker.get_model(n_obs, true_params, seed_obs, stochastic) with the simulation on the device; nodes t1,
    t2, t3, Ricker, Mean, Var, #0, d (stochastic=False: t1, Ricker, Mean, d).  The node Ricker returns the (batch, 3)
    summaries, the Summary nodes pick their column; d is an elfi.Discrepancy over chi_squared (deterministic: elfi.Distance
    over HipDistance('euclidean')).  The observed series is the reference's own simulator with RandomState(seed_obs), reduced
    once with NumPy.  device_priors: t3's uniform prior draws on the device (elfi_amd.priors.uniform); the expon and
    truncnorm priors stay SciPy's."""
    elfi = _elfi()
    from elfi.examples import ricker
    import scipy.stats as ss
    simulator = ricker.stochastic_ricker if stochastic else ricker.ricker
    if true_params is None:
        true_params = [3.8, 0.3, 10.] if stochastic else [3.8]
    y = simulator(*true_params, n_obs=n_obs, random_state=np.random.RandomState(seed_obs))
    obs = np.column_stack([np.mean(y, axis=1), np.var(y, axis=1), ricker.num_zeros(y)]).astype(np.float64)
    m = elfi.ElfiModel()
    from . import priors
    if stochastic:
        elfi.Prior(ss.expon, np.e, 2, model=m, name='t1')
        elfi.Prior(ss.truncnorm, 0, 5, model=m, name='t2')
        elfi.Prior(priors.uniform if device_priors else ss.uniform, 0, 100, model=m, name='t3')
        elfi.Simulator(partial(ricker_summary_rows, n_obs=n_obs), m['t1'], m['t2'], m['t3'], observed=obs, name='Ricker')
        sumstats = [elfi.Summary(partial(column, j=k), m['Ricker'], name=name) for k, name in enumerate(RICKER_NAMES)]
        elfi.Discrepancy(chi_squared, *sumstats, name='d')
    else:
        elfi.Prior(ss.expon, np.e, model=m, name='t1')
        elfi.Simulator(partial(ricker_summary_rows, n_obs=n_obs), m['t1'], observed=obs, name='Ricker')
        mean = elfi.Summary(partial(column, j=0), m['Ricker'], name='Mean')
        elfi.Distance(HipDistance('euclidean'), mean, name='d')
    return m


def lv_summary_rows(r1, r2, r3, prey_init=50, predator_init=100, sigma=None, n_obs=16, time_end=30., max_events=1 << 20,
                    batch_size=1, random_state=None):
    """Simulator operation: (batch, 9) summaries of Lotka-Volterra trajectories simulated, observed and reduced on the
    device (sigma None: no observation noise)."""
    params = (r1, r2, r3, prey_init, predator_init) + (() if sigma is None else (sigma,))
    params = _per_simulation(batch_size, *params)
    return lotka_volterra_summaries(*params, n_obs=n_obs, time_end=time_end, max_events=max_events,
                                    seed=_seed_of(random_state), stream=SIMULATOR_STREAM_BASE)


def lotka_volterra_model(n_obs=50, true_params=None, observation_noise=False, seed_obs=None, device_priors=True, **kwargs):
    """elfi.examples.lotka_volterra.get_model(n_obs, true_params, observation_noise, seed_obs, **kwargs) with the simulation
    on the device; nodes r1, r2, r3, prey0, predator0 [, sigma], LV, the nine summaries LV_NAMES, d.  The node LV returns
    the (batch, 9) summaries, the Summary nodes pick their column; d is elfi.Distance over HipDistance('euclidean').  kwargs
    go to the simulator (time_end, max_events; prey_init and the like are parameters).  The observed series is the
    reference's own simulator with RandomState(seed_obs), reduced once with the reference's summary functions.
    device_priors: the ExpUniform priors draw on the device (elfi_amd.priors.ExpUniform); the normal priors stay SciPy's."""
    if true_params is None:
        true_params = [1.0, 0.005, 0.6, 50, 100, 10.] if observation_noise else [1.0, 0.005, 0.6, 50, 100, 0.]
    elif observation_noise:
        if len(true_params) != 6:
            raise ValueError("Option observation_noise = True. Provide six input parameters.")
    else:
        if len(true_params) != 5:
            raise ValueError("Option observation_noise = False. Provide five input parameters.")
        true_params = list(true_params) + [0]
    elfi = _elfi()
    from elfi.examples import lotka_volterra as lv
    from . import priors
    kwargs = dict(kwargs, n_obs=n_obs)
    ref_kwargs = {k: v for k, v in kwargs.items() if k != 'max_events'}
    y = lv.lotka_volterra(*true_params, random_state=np.random.RandomState(seed_obs), **ref_kwargs)
    fns = [partial(lv.stock_mean, species=0), partial(lv.stock_mean, species=1), partial(lv.stock_log_variance, species=0),
           partial(lv.stock_log_variance, species=1), partial(lv.stock_autocorr, species=0, lag=1),
           partial(lv.stock_autocorr, species=1, lag=1), partial(lv.stock_autocorr, species=0, lag=2),
           partial(lv.stock_autocorr, species=1, lag=2), lv.stock_crosscorr]
    obs = np.column_stack([f(y) for f in fns]).astype(np.float64)
    m = elfi.ElfiModel()
    exp_uniform = priors.ExpUniform if device_priors else lv.ExpUniform
    nodes = [elfi.Prior(exp_uniform, -6., 2., model=m, name='r1'),
             elfi.Prior(exp_uniform, -6., 2., model=m, name='r2'),
             elfi.Prior(exp_uniform, -6., 2., model=m, name='r3'),
             elfi.Prior('normal', 50, np.sqrt(50), model=m, name='prey0'),
             elfi.Prior('normal', 100, np.sqrt(100), model=m, name='predator0')]
    if observation_noise:
        nodes.append(elfi.Prior(exp_uniform, np.log(0.5), np.log(50), model=m, name='sigma'))
    elfi.Simulator(partial(lv_summary_rows, **kwargs), *nodes, observed=obs, name='LV')
    sumstats = [elfi.Summary(partial(column, j=k), m['LV'], name=name) for k, name in enumerate(LV_NAMES)]
    elfi.Distance(HipDistance('euclidean'), *sumstats, name='d')
    return m


def daycare_summary_rows(t1, t2, t3, n_dcc=29, n_ind=53, n_strains=33, freq_strains_commun=None, n_obs=36, time_end=10.,
                         max_events=1 << 16, batch_size=1, random_state=None):
    """Simulator operation: (batch, 4, n_dcc) summaries of day-care centres simulated and reduced on the device."""
    t1, t2, t3 = _per_simulation(batch_size, t1, t2, t3)
    return daycare_summaries(t1, t2, t3, n_dcc=n_dcc, n_ind=n_ind, n_strains=n_strains, freq_strains_commun=freq_strains_commun,
                             n_obs=n_obs, time_end=time_end, max_events=max_events, seed=_seed_of(random_state),
                             stream=SIMULATOR_STREAM_BASE)


def daycare_model(true_params=None, seed_obs=None, device_priors=True, **kwargs):
    """elfi.examples.daycare.get_model(true_params, seed_obs, **kwargs) with the simulation on the device; nodes t1, t2, t3,
    DCC, Shannon, n_strains, prevalence, multi, d, logd.  The node DCC returns the (batch, 4, n_dcc) summaries, the Summary
    nodes pick their (batch, n_dcc) slice; d is an elfi.Discrepancy over elfi_amd.daycare_distance and logd = log d.  kwargs go
    to the simulator (n_dcc, n_ind, n_strains, freq_strains_commun, n_obs, time_end, max_events).  The observed state is the
    reference's own simulator with RandomState(seed_obs), reduced once with the reference's summary functions.
    device_priors: the uniform priors draw on the device (elfi_amd.priors.uniform)."""
    if true_params is None:
        true_params = [3.6, 0.6, 0.1]
    if len(true_params) != 3:
        raise ValueError('true_params must be [t1, t2, t3]')
    elfi = _elfi()
    from elfi.examples import daycare as dc
    from . import priors
    ref_kwargs = {k: v for k, v in kwargs.items() if k != 'max_events'}
    y = dc.daycare(*true_params, random_state=np.random.RandomState(seed_obs), **ref_kwargs)
    fns = [dc.ss_shannon, dc.ss_strains, dc.ss_prevalence, dc.ss_prevalence_multi]
    obs = np.stack([f(y) for f in fns], axis=1).astype(np.float64)            # (1, 4, n_dcc)
    m = elfi.ElfiModel()
    uniform = priors.uniform if device_priors else 'uniform'
    nodes = [elfi.Prior(uniform, 0, 11, model=m, name='t1'),
             elfi.Prior(uniform, 0, 2, model=m, name='t2'),
             elfi.Prior(uniform, 0, 1, model=m, name='t3')]
    elfi.Simulator(partial(daycare_summary_rows, **kwargs), *nodes, observed=obs, name='DCC')
    sumstats = [elfi.Summary(partial(column, j=k), m['DCC'], name=name) for k, name in enumerate(DAYCARE_NAMES)]
    elfi.Discrepancy(daycare_distance, *sumstats, name='d')
    elfi.Operation(np.log, m['d'], name='logd')
    return m


def toad_summary_rows(alpha, gamma, p0, n_toads=66, n_days=63, batch_size=1, random_state=None):
    """Simulator operation: (batch, 48) summaries S1 | S2 | S4 | S8 of toad movements drawn, walked, sorted and reduced on the
    device."""
    alpha, gamma, p0 = _per_simulation(batch_size, alpha, gamma, p0)
    return toad_summaries(alpha, gamma, p0, n_toads=n_toads, n_days=n_days, seed=_seed_of(random_state),
                          stream=SIMULATOR_STREAM_BASE)


def toad_model(true_params=None, seed_obs=None, device_priors=True):
    """elfi.examples.toad.get_model(true_params, seed_obs) with the simulation on the device; nodes alpha, gamma, p0, toad,
    S1, S2, S4, S8, d.  The node toad returns the (batch, 48) summaries of the four lags, the Summary nodes slice their 12
    columns; d is elfi.Distance over HipDistance('euclidean') (as in the reference the example is written for BSL: a
    summary may be inf, and d is not what it is tested on).  The observed positions are the reference's own simulator with
    RandomState(seed_obs), reduced once with the reference's compute_summaries.  device_priors: the three uniform priors draw
    on the device (elfi_amd.priors.uniform)."""
    if true_params is None:
        true_params = [1.7, 35.0, 0.6]
    if len(true_params) != 3:
        raise ValueError('true_params must be [alpha, gamma, p0]')
    elfi = _elfi()
    from elfi.examples import toad
    from . import priors
    y = toad.toad(*true_params, random_state=np.random.RandomState(seed_obs))
    obs = np.hstack([toad.compute_summaries(y, lag) for lag in TOAD_LAGS]).astype(np.float64)     # (1, 48)
    width = obs.shape[1] // len(TOAD_LAGS)
    m = elfi.ElfiModel()
    uniform = priors.uniform if device_priors else 'uniform'
    nodes = [elfi.Prior(uniform, 1, 1, model=m, name='alpha'),
             elfi.Prior(uniform, 0, 100, model=m, name='gamma'),
             elfi.Prior(uniform, 0, 0.9, model=m, name='p0')]
    elfi.Simulator(toad_summary_rows, *nodes, observed=obs, name='toad')
    sumstats = [elfi.Summary(partial(columns, start=k * width, stop=(k + 1) * width), m['toad'], name='S%d' % lag)
                for k, lag in enumerate(TOAD_LAGS)]
    elfi.Distance(HipDistance('euclidean'), *sumstats, name='d')
    return m


def sv_rows(alpha, beta, kappa, eta, mu, phi, sigma, n_obs=50, batch_size=1, random_state=None):
    """Simulator operation: (batch, n_obs + 2) -- the returns of the alpha-stable stochastic-volatility model, then kurt, then
    skew, drawn, chained, sorted and reduced on the device."""
    params = _per_simulation(batch_size, alpha, beta, kappa, eta, mu, phi, sigma)
    S, y = sv_summaries(*params, n_obs=n_obs, seed=_seed_of(random_state), stream=SIMULATOR_STREAM_BASE, return_series=True)
    return np.hstack([y, S])


def sv_model(n_obs=50, true_params=None, seed_obs=None, device_priors=True):
    """elfi.examples.stochastic_volatility_model.get_model(n_obs, true_params, seed_obs) with the simulation on the device;
    nodes alpha, beta, the constants kappa, eta, mu, phi, sigma, a_svm, kurt, skew, d -- and returns.  The node a_svm returns
    (batch, n_obs + 2): the series, then kurt, then skew; the Summary nodes returns, kurt and skew slice its columns (returns
    is what semiBSL is run on in Priddle and Drovandi's paper); d is elfi.Distance over HipDistance('euclidean') of kurt and
    skew.  The observed series is the reference's own simulator with RandomState(seed_obs), reduced once with the
    reference's kurt and skew.  device_priors: the two uniform priors draw on the device (elfi_amd.priors.uniform)."""
    if true_params is None:
        true_params = [1.2, 0.5]
    if len(true_params) != 2:
        raise ValueError('true_params must be [alpha, beta]')
    n_obs = int(n_obs)
    elfi = _elfi()
    from elfi.examples import stochastic_volatility_model as svm
    from . import priors
    fixed = {'kappa': 1, 'eta': 0, 'mu': 0, 'phi': 0.95, 'sigma': 0.2}
    y = svm.alpha_stochastic_volatility_model(*true_params, **fixed, n_obs=n_obs, random_state=np.random.RandomState(seed_obs))
    obs = np.hstack([y, np.reshape(svm.kurt(y), (1, 1)), np.reshape(svm.skew(y), (1, 1))]).astype(np.float64)    # (1, n_obs + 2)
    m = elfi.ElfiModel()
    uniform = priors.uniform if device_priors else 'uniform'
    nodes = [elfi.Prior(uniform, 0.5, 1.5, model=m, name='alpha'),
             elfi.Prior(uniform, -1, 2, model=m, name='beta')]
    nodes += [elfi.Constant(value, model=m, name=name) for name, value in fixed.items()]
    elfi.Simulator(partial(sv_rows, n_obs=n_obs), *nodes, observed=obs, name='a_svm')
    elfi.Summary(partial(columns, start=0, stop=n_obs), m['a_svm'], name='returns')
    kurt = elfi.Summary(partial(column, j=n_obs), m['a_svm'], name='kurt')
    skew = elfi.Summary(partial(column, j=n_obs + 1), m['a_svm'], name='skew')
    elfi.Distance(HipDistance('euclidean'), kurt, skew, name='d')
    return m


def scratch_assay_rows(pm, pp, init_arr, batch_size=1, random_state=None):
    """Simulator operation: (batch, n_obs + 1) summaries of scratch assays walked and reduced on the device."""
    pm, pp = _per_simulation(batch_size, pm, pp)
    return scratch_assay_summaries(pm, pp, init_arr, seed=_seed_of(random_state), stream=SIMULATOR_STREAM_BASE)


def scratch_assay_model(true_params=None, init_arr=None, init_params=None, seed_obs=None, device_priors=True):
    """elfi.examples.scratch_assay.get_model(true_params, init_arr, init_params, seed_obs) with the simulation on the device;
    nodes pm, pp, sim, sums, d.  The node sim returns the (batch, 145) summaries of Price et al. (the reference's sim returns
    the frames and its sums reduces them on the host); the Summary node sums hands them on, and d is elfi.Distance over
    HipDistance('euclidean', w=weis) with the reference's weights.  The observed frames are the reference's own cell_sim with
    RandomState(seed_obs) -- which also draws the initial grid when init_arr is None -- reduced once with the reference's
    cell_summaries.  The grid holds at most 1024 cells.  device_priors: the two uniform priors draw on the device
    (elfi_amd.priors.uniform).

    elfi.BSL(m, ..., feature_names=['sums']) runs this model under the reference's host likelihood; elfi_amd.HipBSL takes a
    Summary of at most 64 columns and refuses the 145 of sums."""
    if true_params is None:
        true_params = [0.25, 0.002]
    if len(true_params) != 2:
        raise ValueError('true_params must be [pm, pp]')
    elfi = _elfi()
    from elfi.examples import scratch_assay as sa
    from . import priors
    obs = sa.cell_sim(*true_params, init_arr, init_params, random_state=np.random.RandomState(seed_obs))
    init = np.ascontiguousarray(obs[:, :, 0], dtype=np.uint8)
    observed = np.asarray(sa.cell_summaries(obs[None, :]), dtype=np.float64)                       # (1, n_obs + 1)
    m = elfi.ElfiModel()
    uniform = priors.uniform if device_priors else 'uniform'
    nodes = [elfi.Prior(uniform, 0, 1, model=m, name='pm'),
             elfi.Prior(uniform, 0, 1, model=m, name='pp')]
    elfi.Simulator(partial(scratch_assay_rows, init_arr=init), *nodes, observed=observed, name='sim')
    elfi.Summary(columns, m['sim'], name='sums')
    num_ds = m['sums'].observed.size - 1
    weis = np.concatenate((np.ones(num_ds) / num_ds, np.array([1]))) / np.sum(init) ** 2
    elfi.Distance(HipDistance('euclidean', w=weis), m['sums'], name='d')
    return m


def bdm_rows(alpha, delta, tau, N, batch_size=1, random_state=None, max_events=1 << 16):
    """Simulator operation: (batch, N) int16 cluster sizes of birth-death-mutation processes run on the device, the shape and
    dtype of the reference's node (which parses its executable's output with np.loadtxt(dtype='int16'))."""
    N = int(np.asarray(N).reshape(-1)[0])
    alpha, delta, tau = _per_simulation(batch_size, alpha, delta, tau)
    return bdm_clusters(alpha, delta, tau, N=N, mode=1, max_events=max_events, seed=_seed_of(random_state),
                        stream=SIMULATOR_STREAM_BASE).astype(np.int16)


def bdm_model(alpha=0.2, delta=0, tau=0.198, N=20, seed_obs=None, max_events=1 << 16, device_priors=True):
    """elfi.examples.bdm.get_model(alpha, delta, tau, N, seed_obs) with the simulation on the device; nodes alpha, BDM, T1,
    d.  No `bdm` executable, no files, no warning.  The node BDM returns the (batch, N) clusters as int16, T1 is the
    reference's own T1 on them, d is elfi.Distance over HipDistance('minkowski', p=1).  With seed_obs None and N == 20 the
    observed data are the clusters of Lintusaari et al. that the reference hard-codes; otherwise they are ONE device simulation
    at (alpha, delta, tau) with seed seed_obs, where the reference would call its binary: a different, equally valid
    realisation.  The parameters reach the simulator as they are; the reference rounds them to 4 decimals in its text file.  A
    simulation is cut off after max_events events (the reference has no bound).  device_priors: the uniform prior draws on the
    device (elfi_amd.priors.uniform)."""
    N = int(N)
    elfi = _elfi()
    from elfi.examples import bdm
    from . import priors
    if seed_obs is None and N == 20:
        y = np.zeros(N, dtype='int16')
        data = np.array([6, 3, 2, 2, 1, 1, 1, 1, 1, 1, 1], dtype='int16')
        y[0:len(data)] = data
    else:
        y = bdm_rows(alpha, delta, tau, N, random_state=np.random.RandomState(seed_obs), max_events=max_events)
    m = elfi.ElfiModel(name='bdm')
    uniform = priors.uniform if device_priors else 'uniform'
    elfi.Prior(uniform, .005, 2, model=m, name='alpha')
    elfi.Simulator(partial(bdm_rows, max_events=max_events), m['alpha'], delta, tau, N, observed=y, name='BDM')
    elfi.Summary(bdm.T1, m['BDM'], name='T1')
    elfi.Distance(HipDistance('minkowski', p=1), m['T1'], name='d')
    return m


def ar1_rows(phi, n_obs=200, batch_size=1, random_state=None):
    """Simulator operation: (batch, n_obs) AR(1) series drawn and chained on the device."""
    phi, = _per_simulation(batch_size, phi)
    return ar1_series(phi, n_obs=n_obs, seed=_seed_of(random_state), stream=SIMULATOR_STREAM_BASE)


def ar1_model(n_obs=200, true_params=None, seed_obs=None, device_priors=True):
    """elfi.examples.ar1.get_model(n_obs, true_params, seed_obs) with the simulation on the device; nodes phi, AR1, d.  The
    node AR1 returns the (batch, n_obs) series and d is elfi.Distance over HipDistance('euclidean') on it.  The observed series
    is the reference's own AR1 with RandomState(seed_obs).  device_priors: the uniform prior draws on the device
    (elfi_amd.priors.uniform)."""
    if true_params is None:
        true_params = [.9]
    if len(true_params) != 1:
        raise ValueError('true_params must be [phi]')
    n_obs = int(n_obs)
    elfi = _elfi()
    from elfi.examples import ar1
    from . import priors
    y = ar1.AR1(*true_params, n_obs=n_obs, random_state=np.random.RandomState(seed_obs))
    m = elfi.ElfiModel()
    uniform = priors.uniform if device_priors else 'uniform'
    elfi.Prior(uniform, -1, 2, model=m, name='phi')
    elfi.Simulator(partial(ar1_rows, n_obs=n_obs), m['phi'], observed=y, name='AR1')
    elfi.Distance(HipDistance('euclidean'), m['AR1'], name='d')
    return m


def gauss_wide_rows(mu, scale=None, batch_size=1, random_state=None):
    """Simulator operation of the wide synthetic Gaussian model: (batch, m) rows mu[:, None] + scale * z, drawn on the device."""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    if mu.shape[0] == 1 and batch_size > 1:
        mu = np.repeat(mu, batch_size)
    return randn_rows(mu, scale, seed=_seed_of(random_state), stream=SIMULATOR_STREAM_BASE)


def gauss_wide_model(m=64, adaptive=True):
    """BASELINE configs[3]'s model: one location parameter mu ~ U(-10, 10), a synthetic Gaussian simulator with m summaries of
    standard deviations 1 .. 20 drawn ON THE DEVICE, observed zeros; the discrepancy node is a HipAdaptiveDistance over the
    simulator's (batch, m) output (adaptive=False: elfi.Distance(HipDistance('euclidean'))).  Nodes mu, sim, d."""
    elfi = _elfi()
    from .adaptive import hip_adaptive_distance_class
    mdl = elfi.new_model()
    from . import priors
    mu = elfi.Prior(priors.uniform, -10, 20, model=mdl, name='mu')      # (ss.uniform with the draws on the device)
    sim = elfi.Simulator(partial(gauss_wide_rows, scale=np.linspace(1.0, 20.0, m)), mu, observed=np.zeros((1, m)), name='sim')
    if adaptive:
        hip_adaptive_distance_class()(sim, name='d')
    else:
        elfi.Distance(HipDistance('euclidean'), sim, name='d')
    return mdl
