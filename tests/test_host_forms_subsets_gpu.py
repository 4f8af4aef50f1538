"""GPU: what a host-pointer entry point of the example simulators returns in one array does not depend on which of its other
optional arrays the caller asked for.

A host form stages its arrays through the context's `in` and `out` buffers (csrc/host_stage.hpp): an array that is not asked
for takes no room there, so every combination of optional arrays is another carving of the buffers.  Each model below is
called through the C ABI with every optional output asked for, then with none, then with each one alone (outputs that the ABI
only takes together, the echoed draws of the toad and stochastic-volatility models, count as one), on the same seed or the
same given draws: every array a call returns must equal the all-outputs call's array -- np.array_equal with NaNs compared
equal, integer arrays exactly.  Every output array starts as a fill pattern, so an array that was never copied back differs too.
The forms of a model are its combinations of optional INPUTS (draws made in the kernel or given, the optional parameters).
The samplers whose only optional arrays are inputs (the stable laws on given angles and exponentials) are compared with
themselves one element at a time instead.

The shapes are the smallest at which the carving can go wrong: a batch of 3 (odd, so that a 4-byte block has an odd count),
series of 3 to 5 values, 64 events.  What each model computes is pinned by its own test file.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 3
U64, DBL = C.c_uint64, C.c_double
SEED, STREAM = U64(7), U64(2)
_rs = np.random.RandomState(31)


def p(a):
    return None if a is None else a.ctypes.data


def f8(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def filled(shape, dtype):
    """an output array before the call: every byte 0x5A"""
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8).fill(0x5A)
    return a


class Model:
    """outputs: {name: (shape, dtype)} in the ABI's order; required: always asked for; units: optional outputs asked for
    together, one name each unless listed; forms: {name: (inputs, names of the outputs the form does not have)};
    call(ctx, inputs, out) makes the call, out[name] an array or None."""

    def __init__(self, name, outputs, call, forms, required=(), units=()):
        self.name, self.outputs, self.call, self.forms, self.required = name, outputs, call, forms, tuple(required)
        grouped = {n for u in units for n in u}
        self.units = [u for u in units] + [(n,) for n in outputs if n not in grouped and n not in required]

    def run(self, ctx, form, asked):
        inputs, absent = self.forms[form]
        out = {}
        for name, (shape, dtype) in self.outputs.items():
            want = (name in self.required or name in asked) and name not in absent
            out[name] = filled(shape, dtype) if want else None
        self.call(ctx, inputs, out)
        return {k: v for k, v in out.items() if v is not None}

    def subsets(self, form):
        absent = self.forms[form][1]
        units = [u for u in self.units if not set(u) & set(absent)]
        return [()] + [u for u in units]


def same(a, b):
    if a.dtype.kind == 'f':
        return np.array_equal(a, b, equal_nan=True)
    return np.array_equal(a, b)


# ---- ARCH(1), AR(1), M/G/1, Ricker (csrc/series.hip) ------------------------------------------------------------------
N_OBS, N_LAGS, NQ = 5, 2, 3
ARCH_M = 2 + N_LAGS + N_LAGS * (N_LAGS - 1) // 2
T1, T2, T3 = f8(_rs.uniform(-0.9, 0.9, B)), f8(_rs.uniform(0.1, 0.9, B)), f8(_rs.uniform(0.1, 0.5, B))
SRV_LO = f8(_rs.uniform(0, 2, B))
SRV_HI = f8(SRV_LO + _rs.uniform(1, 3, B))


def quantile_positions(q, n):
    from elfi_amd.summaries import quantile_positions as qp
    return [np.ascontiguousarray(a) for a in qp(q, n)]


def arch_call(ctx, i, o):
    ctx.call('elfihip_arch_summaries', p(i['W']), SEED, STREAM, B, N_OBS, N_LAGS, p(T1), p(T2), p(i['obs']), p(o['S']), p(o['Y']),
             p(o['D']))


ARCH_OBS = f8(_rs.randn(ARCH_M))
ARCH = Model('arch', dict(S=((B, ARCH_M), 'f8'), Y=((B, N_OBS), 'f8'), D=((B,), 'f8')), arch_call,
             dict(drawn=(dict(W=None, obs=ARCH_OBS), ()), given=(dict(W=f8(_rs.randn(B, N_OBS + 2)), obs=ARCH_OBS), ())),
             required=('S',))


def ar1_call(ctx, i, o):
    ctx.call('elfihip_ar1_series', p(i['W']), SEED, STREAM, B, N_OBS, p(T1), p(i['obs']), p(o['X']), p(o['D']))


AR1_OBS = f8(_rs.randn(N_OBS))
AR1 = Model('ar1', dict(X=((B, N_OBS), 'f8'), D=((B,), 'f8')), ar1_call,
            dict(drawn=(dict(W=None, obs=AR1_OBS), ()), given=(dict(W=f8(_rs.randn(B, N_OBS + 1)), obs=AR1_OBS), ())))


def mg1_call(ctx, i, o):
    lo, hi, t = quantile_positions([0.25, 0.5, 0.75], N_OBS)
    ctx.call('elfihip_mg1_summaries', p(i['E']), p(i['V']), SEED, STREAM, B, N_OBS, p(SRV_LO), p(SRV_HI), p(T3), NQ, p(lo), p(hi),
             p(t), p(i['obs']), None, p(o['logY']), p(o['Q']), p(o['Y']), p(o['Eo']), p(o['Vo']), p(o['D']))


MG1_OBS = f8(_rs.uniform(1, 5, NQ))
MG1 = Model('mg1', dict(logY=((B, N_OBS), 'f8'), Q=((B, NQ), 'f8'), Y=((B, N_OBS), 'f8'), Eo=((B, N_OBS), 'f8'),
                        Vo=((B, N_OBS), 'f8'), D=((B,), 'f8')), mg1_call,
            dict(drawn=(dict(E=None, V=None, obs=MG1_OBS), ()),
                 given=(dict(E=f8(_rs.exponential(1.0, (B, N_OBS))), V=f8(_rs.uniform(0, 1, (B, N_OBS))), obs=MG1_OBS), ())),
            required=('logY', 'Q'))


def ricker_call(ctx, i, o):
    ctx.call('elfihip_ricker_summaries', p(i['Z']), SEED, STREAM, B, N_OBS, p(i['log_rate']), p(i['sd']), p(i['scale']), DBL(1.0),
             p(i['obs']), 0, p(o['S']), p(o['Y']), p(o['St']), p(o['Zo']), p(o['D']))


_RK = dict(log_rate=f8(_rs.uniform(3, 4, B)), sd=f8(_rs.uniform(0.1, 0.5, B)), scale=f8(_rs.uniform(5, 15, B)),
           obs=f8([40.0, 3600.0, 2.0]))
RICKER = Model('ricker', dict(S=((B, 3), 'f8'), Y=((B, N_OBS), 'f8'), St=((B, N_OBS), 'f8'), Zo=((B, N_OBS), 'f8'), D=((B,), 'f8')),
               ricker_call,
               dict(drawn=(dict(_RK, Z=None), ()), given=(dict(_RK, Z=f8(_rs.randn(B, N_OBS))), ()),
                    deterministic=(dict(_RK, Z=None, sd=None, scale=None), ('Zo',))),
               required=('S',))

# ---- g-and-k (csrc/gnk.hip) ---------------------------------------------------------------------------------------------
GNK_OBS_N = 4


def gnk_model(dim):
    L, npar = GNK_OBS_N * dim, 4 if dim == 1 else 9
    P = f8(_rs.uniform(0.5, 3, (B, npar)))
    if dim == 2:
        P[:, 8] = _rs.uniform(-0.9, 0.9, B)
    obs = f8(_rs.uniform(0, 5, 7 * dim))

    def call(ctx, i, o):
        lo, hi, t = quantile_positions(np.true_divide(np.linspace(12.5, 87.5, 7), 100), GNK_OBS_N)
        ctx.call('elfihip_gnk_summaries', p(i['Z']), SEED, STREAM, B, GNK_OBS_N, dim, p(P), DBL(0.8), p(lo), p(hi), p(t), p(obs), 2,
                 p(o['Y']), p(o['Zo']), p(o['Ys']), p(o['O']), p(o['R']), p(o['D']))

    return Model('gnk%d' % dim, dict(Y=((B, L), 'f8'), Zo=((B, L), 'f8'), Ys=((B, L), 'f8'), O=((B, 7 * dim), 'f8'),
                                     R=((B, 4 * dim), 'f8'), D=((B,), 'f8')), call,
                 dict(drawn=(dict(Z=None), ()), given=(dict(Z=f8(_rs.randn(B, L))), ())))


# ---- Lorenz-96 (csrc/lorenz.hip) ----------------------------------------------------------------------------------------
LZ_K, LZ_T = 4, 3


def lorenz_call(ctx, i, o):
    ctx.call('elfihip_lorenz_summaries', p(i['E']), SEED, STREAM, B, LZ_K, LZ_T, p(i['t1']), p(i['t2']), DBL(10.0), DBL(0.178),
             DBL(0.984), DBL(0.025), p(i['y0']), int(i['y0'].ndim == 2), p(i['obs']), p(o['S']), p(o['Y']), p(o['D']))


_LZ = dict(t1=f8(_rs.uniform(0.5, 3.5, B)), t2=f8(_rs.uniform(0, 0.3, B)), obs=f8(_rs.randn(6)))
LORENZ = Model('lorenz', dict(S=((B, 6), 'f8'), Y=((B, LZ_T * LZ_K), 'f8'), D=((B,), 'f8')), lorenz_call,
               dict(drawn_shared_start=(dict(_LZ, E=None, y0=f8(3.0 * _rs.randn(LZ_K))), ()),
                    given_own_start=(dict(_LZ, E=f8(_rs.randn(B, (LZ_T - 1) * LZ_K)), y0=f8(3.0 * _rs.randn(B, LZ_K))), ())),
               required=('S',))

# ---- the toad model (csrc/toad.hip) -------------------------------------------------------------------------------------
TOADS, DAYS = 3, 4
TOAD_CELLS = (DAYS - 1) * TOADS
TOAD_LAGS = np.array([1, 2], dtype=np.int32)
TOAD_P = f8([0.0, 0.5, 1.0])
TOAD_NS = (TOAD_P.shape[0] + 1) * TOAD_LAGS.shape[0]
_TD = [f8(_rs.uniform(1.2, 1.9, B)), f8(_rs.uniform(10, 50, B)), f8(_rs.uniform(0.2, 0.8, B))]


def toad_call(ctx, i, o):
    ctx.call('elfihip_toad_summaries', p(i['U']), p(i['TH']), p(i['W']), p(i['R']), SEED, STREAM, 0, B, TOADS, DAYS,
             TOAD_LAGS.shape[0], p(TOAD_LAGS), TOAD_P.shape[0], p(TOAD_P), DBL(10.0), p(_TD[0]), p(_TD[1]), p(_TD[2]), p(o['S']),
             p(o['X']), p(o['Dx']), p(o['Uo']), p(o['THo']), p(o['Wo']), p(o['Ro']))


_TOAD_R = np.ascontiguousarray(np.stack([_rs.randint(0, day, (B, TOADS)) for day in range(1, DAYS)], axis=1), dtype=np.int32)
TOAD = Model('toad', dict(S=((B, TOAD_NS), 'f8'), X=((B, DAYS * TOADS), 'f8'), Dx=((B, TOAD_CELLS), 'f8'), Uo=((B, TOAD_CELLS), 'f8'),
                          THo=((B, TOAD_CELLS), 'f8'), Wo=((B, TOAD_CELLS), 'f8'), Ro=((B, TOAD_CELLS), 'i4')), toad_call,
             dict(drawn=(dict(U=None, TH=None, W=None, R=None), ()),
                  given=(dict(U=f8(_rs.uniform(0, 1, (B, TOAD_CELLS))), TH=f8(_rs.uniform(-1.5, 1.5, (B, TOAD_CELLS))),
                              W=f8(_rs.exponential(1.0, (B, TOAD_CELLS))), R=_TOAD_R.reshape(B, TOAD_CELLS)), ())),
             required=('S',), units=[('Uo', 'THo', 'Wo', 'Ro')])

# ---- stochastic volatility (csrc/sv.hip) ----------------------------------------------------------------------------------
SV_OBS = 3
SV_Q = f8([.05, .25, .75, .95, .05, .5, .95])
_SV = [f8(_rs.uniform(1.2, 1.9, B)), f8(_rs.uniform(-0.5, 0.5, B)), f8(np.ones(B)), f8(np.zeros(B)), f8(np.zeros(B)),
       f8(np.full(B, 0.95)), f8(np.full(B, 0.2))]


def sv_call(ctx, i, o):
    ctx.call('elfihip_sv_summaries', p(i['Z']), p(i['TH']), p(i['W']), SEED, STREAM, 0, B, SV_OBS, p(SV_Q), *[p(a) for a in _SV],
             p(i['x0']), p(o['S']), p(o['Y']), p(o['X']), p(o['V']), p(o['Zo']), p(o['THo']), p(o['Wo']))


SV = Model('sv', dict(S=((B, 2), 'f8'), Y=((B, SV_OBS), 'f8'), X=((B, SV_OBS), 'f8'), V=((B, SV_OBS), 'f8'), Zo=((B, SV_OBS), 'f8'),
                      THo=((B, SV_OBS), 'f8'), Wo=((B, SV_OBS), 'f8')), sv_call,
           dict(drawn_stationary=(dict(Z=None, TH=None, W=None, x0=None), ()),
                given_with_start=(dict(Z=f8(_rs.randn(B, SV_OBS)), TH=f8(_rs.uniform(-1.5, 1.5, (B, SV_OBS))),
                                       W=f8(_rs.exponential(1.0, (B, SV_OBS))), x0=f8(_rs.randn(B))), ())),
           required=('S',), units=[('Zo', 'THo', 'Wo')])

# ---- the event-driven simulators (csrc/gillespie.hip, daycare.hip, scratch_assay.hip, bdm.hip) ------------------------------
EVENTS = 64
LV_OBS = 3
_LV = [f8(_rs.uniform(0.8, 1.2, B)), f8(_rs.uniform(0.004, 0.006, B)), f8(_rs.uniform(0.5, 0.7, B)), f8(np.full(B, 5.0)),
       f8(np.full(B, 10.0))]


def lv_call(ctx, i, o):
    ctx.call('elfihip_lv_summaries', p(i['E']), p(i['U']), p(i['Z']), SEED, STREAM, 0, B, LV_OBS, DBL(2.0), EVENTS,
             *[p(a) for a in _LV], p(i['sigma']), p(i['obs']), p(o['Y']), p(o['T']), p(o['status']), p(o['events']), p(o['S']),
             p(o['D']))


_LV_OBS = f8(np.arange(1.0, 10.0))
_LV_SIGMA = f8(_rs.uniform(0.5, 2.0, B))
LV = Model('lv', dict(Y=((B, 2 * LV_OBS), 'f8'), T=((B,), 'f8'), status=((B,), 'i4'), events=((B,), 'i8'), S=((B, 9), 'f8'),
                      D=((B,), 'f8')), lv_call,
           dict(drawn=(dict(E=None, U=None, Z=None, sigma=None, obs=_LV_OBS), ()),
                drawn_noisy=(dict(E=None, U=None, Z=None, sigma=_LV_SIGMA, obs=_LV_OBS), ()),
                given_noisy=(dict(E=f8(_rs.exponential(1.0, (B, EVENTS))), U=f8(_rs.uniform(0, 1, (B, EVENTS))),
                                  Z=f8(_rs.randn(B, 2 * (LV_OBS - 1))), sigma=_LV_SIGMA, obs=_LV_OBS), ())))

DCC, IND, STRAINS = 2, 3, 2
_DC = [f8(_rs.uniform(2.0, 5.0, B)), f8(_rs.uniform(0.3, 0.9, B)), f8(_rs.uniform(0.05, 0.3, B))]
_DC_OBS = f8(_rs.uniform(0.1, 1.0, (4, DCC)))


def daycare_call(ctx, i, o):
    ctx.call('elfihip_daycare_summaries', p(i['E']), p(i['U']), SEED, STREAM, 0, B, DCC, IND, STRAINS, IND, DBL(1.0), EVENTS,
             *[p(a) for a in _DC], None, p(_DC_OBS), p(o['M']), p(o['T']), p(o['status']), p(o['events']), p(o['S']), p(o['D']))


DAYCARE = Model('daycare', dict(M=((B, DCC, IND), 'u8'), T=((B, DCC), 'f8'), status=((B, DCC), 'i4'), events=((B, DCC), 'i8'),
                                S=((B, 4, DCC), 'f8'), D=((B,), 'f8')), daycare_call,
                dict(drawn=(dict(E=None, U=None), ()),
                     given=(dict(E=f8(_rs.exponential(1.0, (B, DCC, EVENTS))), U=f8(_rs.uniform(0, 1, (B, DCC, EVENTS)))), ())))

SA_ROWS = SA_COLS = 2
SA_ITER, SA_EVERY = 4, 2
SA_INIT = np.array([[1, 0], [0, 1]], dtype=np.uint8)
_SA = [f8(_rs.uniform(0.2, 1.0, B)), f8(_rs.uniform(0.0, 0.5, B))]
_SA_SHAPE = (B, SA_ITER, 2, SA_ROWS * SA_COLS)


def assay_call(ctx, i, o):
    ctx.call('elfihip_assay_summaries', p(i['C']), p(i['P']), p(i['M']), SEED, STREAM, 0, B, SA_ROWS, SA_COLS, SA_ITER, SA_EVERY,
             p(SA_INIT), p(_SA[0]), p(_SA[1]), p(o['S']), p(o['status']), p(o['events']), p(o['frames']))


ASSAY = Model('assay', dict(S=((B, SA_ITER // SA_EVERY + 1), 'f8'), status=((B,), 'i4'), events=((B, 2), 'i8'),
                            frames=((B, SA_ITER // SA_EVERY + 1, 32), 'u4')), assay_call,
              dict(drawn=(dict(C=None, P=None, M=None), ()),
                   # candidate 0 is valid whatever the cell count
                   given=(dict(C=np.zeros(_SA_SHAPE, dtype=np.int32), P=f8(_rs.uniform(0, 1, _SA_SHAPE)),
                               M=np.ascontiguousarray(_rs.randint(0, 4, _SA_SHAPE), dtype=np.uint8)), ())),
              required=('S',))

BD_N = 4
_BD = [f8(_rs.uniform(0.5, 1.5, B)), f8(_rs.uniform(0.0, 0.3, B)), f8(_rs.uniform(0.05, 0.5, B))]
_BD_OBS = f8([0.4])


def bdm_call(ctx, i, o):
    ctx.call('elfihip_bdm_clusters', p(i['U']), SEED, STREAM, 0, B, BD_N, 1, EVENTS, *[p(a) for a in _BD], DBL(float(BD_N)),
             p(_BD_OBS), p(o['Cl']), p(o['status']), p(o['events']), p(o['T']), p(o['D']))


BDM = Model('bdm', dict(Cl=((B, BD_N), 'i4'), status=((B,), 'i4'), events=((B,), 'i8'), T=((B, 2), 'f8'), D=((B,), 'f8')), bdm_call,
            dict(drawn=(dict(U=None), ()), given=(dict(U=f8(_rs.uniform(0, 1, (B, 2 * EVENTS)))), ())))

MODELS = [ARCH, AR1, MG1, RICKER, gnk_model(1), gnk_model(2), LORENZ, TOAD, SV, LV, DAYCARE, ASSAY, BDM]
CASES = [(m, form) for m in MODELS for form in m.forms]


@pytest.fixture(scope='module')
def ctx(hip_ctx):
    import elfi_amd
    c = elfi_amd.Context()
    yield c
    c.close()


@pytest.mark.parametrize('model, form', CASES, ids=['%s-%s' % (m.name, f) for m, f in CASES])
def test_an_output_does_not_depend_on_the_outputs_asked_for_with_it(ctx, model, form):
    absent = model.forms[form][1]
    everything = model.run(ctx, form, [n for n in model.outputs if n not in absent])
    assert set(everything) == set(model.outputs) - set(absent)
    for name, a in everything.items():
        assert not np.all(a == filled((1,), a.dtype)[0]), '%s %s: %s was not written by the all-outputs call' % (model.name, form, name)
    for asked in model.subsets(form):
        got = model.run(ctx, form, asked)
        assert set(got) == set(model.required) | set(asked)
        for name, a in got.items():
            assert a.dtype == everything[name].dtype and same(a, everything[name]), \
                '%s %s: %s differs from the all-outputs call when asked for with %s' % (model.name, form, name, asked or 'nothing else')


# ---- the samplers whose optional arrays are inputs (csrc/stable.hip, csrc/stable_general.hip) -------------------------------
def test_stable_laws_on_given_angles_are_the_same_one_element_at_a_time(ctx):
    alpha, beta, loc, scale = f8(_rs.uniform(1.1, 1.9, B)), f8(_rs.uniform(-0.5, 0.5, B)), f8(_rs.randn(B)), f8(_rs.uniform(0.5, 2, B))
    angle, expo = f8(_rs.uniform(-1.5, 1.5, B)), f8(_rs.exponential(1.0, B))

    def stable(sl):
        args, out = [f8(a[sl]) for a in (alpha, scale, angle, expo)], np.full(alpha[sl].shape, np.nan)
        ctx.call('elfihip_stable', SEED, STREAM, out.shape[0], *[p(a) for a in args], p(out))
        return out

    def general(sl):
        args, out = [f8(a[sl]) for a in (alpha, beta, loc, scale, angle, expo)], np.full(alpha[sl].shape, np.nan)
        ctx.call('elfihip_stable_general', SEED, STREAM, out.shape[0], 1, *[p(a) for a in args], p(out))
        return out

    for fn in (stable, general):
        whole = fn(slice(0, B))
        assert np.all(np.isfinite(whole))
        assert np.array_equal(whole, np.concatenate([fn(slice(e, e + 1)) for e in range(B)])), fn.__name__
    # ... and element 0 of the drawn forms is the same in a batch of one and in a batch of three (counter 0 either way)
    for name, pars in (('elfihip_stable', (alpha, scale)), ('elfihip_stable_general', (alpha, beta, loc, scale))):
        outs = []
        for n in (1, B):
            out = np.full(n, np.nan)
            extra = (1,) if name.endswith('general') else ()
            args = [f8(a[:n]) for a in pars]
            ctx.call(name, SEED, STREAM, n, *extra, *[p(a) for a in args], None, None, p(out))
            outs.append(out)
        assert np.isfinite(outs[0][0]) and outs[0][0] == outs[1][0], name
