"""GPU: the four event-driven simulators (csrc/gillespie.hip, daycare.hip, scratch_assay.hip, bdm.hip) share ONE work buffer
and ONE occupancy cache in the context (csrc/event_sim.hpp).  What each computes is pinned by its own test file; this one holds
the sharing: on one context the drawn forms are called in an interleaved order, each twice, and every result must equal, byte
for byte, the same call on a context that has seen nothing else.

The buffer holds the counter at offset 0, a 256-byte head and then the calling model's work space.  Lotka-Volterra without the
series and day-care without state and status but with a distance keep work space behind the head; the scratch assay and
birth-death-mutation need the head alone.  'forward' has the small users follow the large ones, and the large ones follow the
small ones on the way back, in a buffer that is already large enough; 'backward' starts a context with the small users, so
that the large ones that follow make the buffer grow -- twice -- and move the counter.  The shapes are the smallest that still
deal work out: 130 Lotka-Volterra simulations are two full wavefronts and a partial one whose lanes refill and retire, the other
models take several units per call, and birth-death-mutation runs its register instance (N = 20) and its LDS instance (N = 100).
"""
import faulthandler

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_rs = np.random.RandomState(20)
LV_PAR = (_rs.uniform(0.8, 1.2, 130), _rs.uniform(0.004, 0.006, 130), _rs.uniform(0.5, 0.7, 130))
DC_PAR = (_rs.uniform(2.0, 5.0, 3), _rs.uniform(0.3, 0.9, 3), _rs.uniform(0.05, 0.3, 3))
DC_OBS = _rs.uniform(0.1, 1.0, (4, 5))
SA_PAR = (_rs.uniform(0.2, 1.0, 5), _rs.uniform(0.0, 0.2, 5))
SA_GRID = (np.arange(6 * 7).reshape(6, 7) % 3 == 0).astype(np.uint8)
BD_PAR = (_rs.uniform(0.5, 1.5, 70), _rs.uniform(0.0, 0.3, 70), _rs.uniform(0.05, 0.5, 70))


def lv(ea, ctx):
    return ea.lotka_volterra_summaries(*LV_PAR, n_obs=8, time_end=2.0, max_events=300, seed=11, stream=2, observed=np.arange(1.0, 10.0),
                                       return_status=True, ctx=ctx)


def daycare(ea, ctx):
    return ea.daycare_summaries(*DC_PAR, n_dcc=5, time_end=1.0, max_events=4096, seed=12, stream=4, observed=DC_OBS, ctx=ctx)


def assay(ea, ctx):
    return ea.scratch_assay_summaries(*SA_PAR, SA_GRID, obs_period=12, obs_interval=3, tau=1, seed=13, stream=6, return_frames=True,
                                      return_events=True, ctx=ctx)


def bdm(ea, ctx):
    return ea.bdm_clusters(*BD_PAR, N=20, max_events=4096, seed=14, stream=8, observed=[0.4], return_summaries=True,
                           return_status=True, ctx=ctx)


def bdm_wide(ea, ctx):
    return ea.bdm_clusters(*(p[:3] for p in BD_PAR), N=100, max_events=4096, seed=15, stream=10, observed=[0.4],
                           return_summaries=True, return_status=True, ctx=ctx)


CALLS = (lv, daycare, assay, bdm, bdm_wide)


@pytest.fixture(autouse=True)
def time_limit():
    """A hung kernel ends the run instead of holding the device: the process exits after 120 s in one test."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope='module')
def alone(hip_ctx):
    """every call on a context of its own"""
    import elfi_amd
    want = {}
    for call in CALLS:
        ctx = elfi_amd.Context()
        want[call.__name__] = call(elfi_amd, ctx)
        ctx.close()
    events = {'lv': want['lv'][2], 'daycare': None, 'assay': want['assay'][3], 'bdm': want['bdm'][3], 'bdm_wide': want['bdm_wide'][3]}
    for name, ev in events.items():
        assert ev is None or ev.sum() > 0, '%s: no event was made' % name
    return want


@pytest.mark.parametrize('order', ['forward', 'backward'])
def test_interleaved_calls_on_one_context_equal_calls_alone(alone, order):
    import elfi_amd
    there = CALLS if order == 'forward' else CALLS[::-1]
    ctx = elfi_amd.Context()
    for turn, call in enumerate(there + there[::-1]):
        got, want = call(elfi_amd, ctx), alone[call.__name__]
        assert len(got) == len(want)
        for part, (a, b) in enumerate(zip(got, want)):
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), \
                '%s, call %d (%s): output %d differs from the call alone' % (order, turn, call.__name__, part)
    ctx.close()
