"""The `_dev` entry points the way production calls them (include/elfihip.h, elfihip_ctx_set_stream): on ONE adopted,
non-null stream that is busy, behind the producer of their inputs, with no host synchronisation in between.

    with adopted_stream(hip_ctx) as s:          # torch's current stream and the context's stream are one non-null stream
        busy(s, DELAY_MS)                       # ordinary torch work that keeps the stream busy for a while
        late(x, x_real)                         # the inputs get their contents BEHIND that work; until then they are poison
        ... library calls, host arguments overwritten the moment each returns ...
        assert not s.query()                    # nobody waited, and the delay was still pending

A launch on another stream reads the poison, a host argument read after the call returned reads garbage, a hidden host
wait lets the delay run out; `Driver` runs a case this way and the established way (own stream, full synchronisation
around every call) and the test compares the two bit for bit.  A plain module: it defines no fixture.

The harness must not be vacuous: `select_stream` keeps a stream only if a reader on the null stream really OBSERVES the
poison while the delay is pending -- two streams that share a hardware queue serialise, and then a wrong-stream launch
would be invisible.
"""
import contextlib
import time

import numpy as np

from device_layout import SENTINEL, _LEAD, _TAIL

DELAY_MS = 20.0
_MM = 2048                 # one float64 matmul of this size is a few hundred microseconds: long against its launch
_CANDIDATES = 4

_state = {}                # 'stream', 'index', 'mm_ms' (one matmul, measured once), 'mm' (operands), 'control' (text)
REPORT = []                # (case, delay ms enqueued, host issue ms, stream still busy) of every busy run, for the log


def _operands():
    import torch
    if 'mm' not in _state:
        a = torch.full((_MM, _MM), 1.0 / _MM, dtype=torch.float64, device='cuda')
        _state['mm'] = (a, a.clone(), torch.empty_like(a))
    return _state['mm']


def _calibrate(stream):
    """Milliseconds of one matmul on `stream`, by torch events (after a warm-up that also creates the BLAS handle of the
    stream).  Calibrates the harness, not the code under test."""
    import torch
    a, b, c = _operands()
    with torch.cuda.stream(stream):
        for _ in range(3):
            torch.mm(a, b, out=c)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(8):
            torch.mm(a, b, out=c)
        e1.record(stream)
    stream.synchronize()
    return max(e0.elapsed_time(e1) / 8, 1e-3)


def busy(stream, ms=DELAY_MS):
    """Enqueue about `ms` milliseconds of float64 matmuls on `stream` -> the milliseconds enqueued."""
    import torch
    a, b, c = _operands()
    reps = max(1, int(np.ceil(ms / _state['mm_ms'])))
    with torch.cuda.stream(stream):
        for _ in range(reps):
            torch.mm(a, b, out=c)
    return reps * _state['mm_ms']


def late(dst, src):
    """dst <- src in the order of torch's current stream (the adopted one)."""
    dst.copy_(src, non_blocking=True)


def poison_value(dtype):
    import torch
    return float('nan') if dtype in (torch.float64, torch.float32) else 0


def poisoned_like(src):
    """A device tensor of src's shape and type that is NaN (floating point) or 0 (integer draws): what the "invalid rows
    are NaN and alone" tests already feed, so no kernel loops on it."""
    import torch
    return torch.full_like(src, poison_value(src.dtype))


def _control(stream):
    """A null-stream reader of a poisoned buffer whose real contents are enqueued on `stream` behind the delay ->
    (the reader saw nothing but the poison, the stream was still busy when the reader had finished)."""
    import torch
    real = torch.arange(1.0, 4097.0, dtype=torch.float64, device='cuda')
    buf = poisoned_like(real)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        busy(stream)
        late(buf, real)
    null = torch.cuda.default_stream()
    assert null.cuda_stream == 0, 'torch\'s default stream is expected to be the null stream'
    with torch.cuda.stream(null):
        seen = buf.clone()
    null.synchronize()
    pending = not stream.query()
    stream.synchronize()
    assert torch.equal(buf, real), 'the late fill itself did not arrive'
    return bool(torch.isnan(seen).all().item()), pending


def select_stream():
    """The adopted stream of this process: the first of up to four torch streams on which the control observes the poison.
    Raises (the calling test fails; it neither passes nor skips) when none does."""
    import torch
    if 'stream' in _state:
        return _state['stream']
    if 'control' in _state:
        raise AssertionError(_state['control'])
    seen = []
    keep = []                       # (candidates stay alive, so that the next one is a different stream)
    for i in range(_CANDIDATES):
        s = torch.cuda.Stream()
        keep.append(s)
        assert s.cuda_stream != 0
        _state['mm_ms'] = _calibrate(s)
        poison, pending = _control(s)
        seen.append('candidate %d: null-stream reader saw %s, stream %s' %
                    (i, 'the poison' if poison else 'the real data', 'still busy' if pending else 'already idle'))
        if poison and pending:
            _state.update(stream=s, index=i, control='; '.join(seen))
            print('stream_order: %s -> candidate %d adopted; one matmul %.3f ms, delay %.1f ms'
                  % (_state['control'], i, _state['mm_ms'], DELAY_MS))
            return s
    _state['control'] = ('no torch stream is independent of the null stream here, a launch on the wrong stream would go '
                         'unnoticed: ' + '; '.join(seen))
    raise AssertionError(_state['control'])


@contextlib.contextmanager
def adopted_stream(hip_ctx):
    """The selected stream as torch's current stream AND the context's stream; on exit, also on failure, the stream is
    synchronised, the context gets its own stream back and torch its previous one (hip_ctx is session-wide: a leaked
    stream would poison every later test)."""
    import torch
    s = select_stream()
    prev = torch.cuda.current_stream()
    torch.cuda.set_stream(s)
    try:
        hip_ctx.set_stream(s.cuda_stream)
        yield s
    finally:
        try:
            s.synchronize()
        finally:
            hip_ctx.set_stream(None)
            torch.cuda.set_stream(prev)


def clobber(h):
    """Overwrite a host array argument in place: NaN for floating point; ONES for integers (prefixes, lags, quantile
    positions) -- the library checks those on the host before it uploads them, so a late read would hand the kernel
    unchecked values: ones are other values than any case passes and still a valid row bound, lag or position, and a late
    read shows as different bits, not as an access out of bounds."""
    if h.dtype.kind == 'f':
        h.view(np.uint8).reshape(-1)[:] = 0xFF
    else:
        h.reshape(-1)[:] = 1


class Buf:
    """A device buffer of a case: `.ptr` is what the call receives, `.t` the tensor."""

    def __init__(self, t, first=0):
        self.t = t
        self.ptr = t.data_ptr() + first * t.element_size()


class Driver:
    """Runs a case.  The case declares its buffers first, says `go()`, issues its calls, says `done()`:

        x = d.input(X)              device input with these contents (any dtype, any shape; passed flat)
        s = d.inout(S0)             device buffer the call updates in place
        o = d.out(n, K)             n x K doubles between sentinels (device_layout.guarded_out's layout)
        o = d.out_raw(count, dt)    `count` elements of another type, every byte 0xA5
        h = d.host(a)               a private, writeable copy of a host array argument
        d.go()
        d.call('elfihip_..._dev', handle, ..., h.ctypes.data, ..., host=(h,))     # host arrays are clobbered behind it
        d.done()                    end of the part that must not synchronise
        d.keep('name', array)       a host result fetched by a synchronising call after done()

    busy=False: the established way -- private inputs filled and synchronised before (by the same device copy as below, on
    torch's default stream, once the uploads have been checked), the context's own stream, the context synchronised after
    every call.  busy=True: the adopted busy stream of this module, inputs poisoned until their contents arrive behind the
    delay, host arguments overwritten as soon as the call has returned, outputs copied aside and inputs re-poisoned in
    stream order, one synchronisation at the end.  `finish()` -> name -> the bytes of every output and kept result."""

    def __init__(self, hip_ctx, busy_run, name='', syncs=False):
        self.ctx, self.lib, self.cx = hip_ctx, hip_ctx.lib, hip_ctx.handle
        self.busy, self.name, self.syncs = busy_run, name, syncs
        self.fills, self.outs, self.kept, self.cleanup, self._src = [], [], {}, [], []
        self.guarded = []                 # names of the results that lie between sentinels (out)
        self.stream = None
        self.still_busy = None

    # ---- declarations
    def _dev(self, a):
        import torch
        src = np.ascontiguousarray(a).reshape(-1).copy()
        t = torch.from_numpy(src).cuda()
        self._src.append((t, src))            # (the source stays alive until the upload has been checked: go())
        return t

    def input(self, a, first=0):
        real = self._dev(a)
        t = poisoned_like(real)
        self.fills.append((t, real))      # filled in go(): behind the delay (busy), or at once and synchronised (established way)
        return Buf(t, first)

    def inout(self, a):
        b = self.input(a)
        self.outs.append(b.t)
        return b

    def out(self, n, K=1):
        import torch
        t = torch.full((_LEAD + n * K + _TAIL,), SENTINEL, dtype=torch.float64, device='cuda')
        self.guarded.append('out%d' % len(self.outs))
        self.outs.append(t)
        return Buf(t, _LEAD)

    def out_raw(self, count, dtype):
        import torch
        nbytes = count * torch.empty((), dtype=dtype).element_size()
        t = torch.full((nbytes + 64,), 0xA5, dtype=torch.uint8, device='cuda')
        self.outs.append(t)
        return Buf(t)

    def host(self, a):
        return np.array(a, copy=True, order='C')

    # ---- the run
    def go(self):
        import torch
        torch.cuda.synchronize()
        self.ctx.synchronize()
        for t, src in self._src:              # the harness's own uploads: a case must not fail for them
            assert np.array_equal(t.cpu().numpy().view(np.uint8), src.view(np.uint8)), 'an input did not reach the device intact'
        self._src = []
        if not self.busy:                     # in both runs an input comes into being by the same device copy
            for dst, real in self.fills:
                late(dst, real)
            torch.cuda.synchronize()
        if self.busy:
            self._cm = adopted_stream(self.ctx)
            self.stream = self._cm.__enter__()
            try:
                self.delay = busy(self.stream)
                for dst, real in self.fills:
                    late(dst, real)
            except BaseException:
                self._cm.__exit__(None, None, None)
                raise
        self.t0 = time.perf_counter()

    def call(self, fn, *args, host=()):
        rc = getattr(self.lib, fn)(*args)
        if self.busy:
            for h in host:                      # the caller's memory is the caller's again
                clobber(h)
        else:
            self.ctx.synchronize()
        if rc != 0:
            msg = self.lib.elfihip_last_error(self.cx)
            raise AssertionError('%s returned %d: %s' % (fn, rc, msg.decode('utf-8', 'replace') if msg else ''))

    def done(self):
        self.issue_ms = (time.perf_counter() - self.t0) * 1e3
        if self.busy:
            self.still_busy = not self.stream.query()
            REPORT.append((self.name, self.delay, self.issue_ms, self.still_busy))
            print('stream_order: %-34s delay %.1f ms, calls issued in %.3f ms, stream %s'
                  % (self.name, self.delay, self.issue_ms, 'still busy' if self.still_busy else 'IDLE'))

    def fetch(self, dst, ptr, count):
        """`count` 8-byte words at the device address `ptr` (memory the library owns and hands out) -> the start of the
        results of `dst`, by a device copy in the order of torch's current stream: the adopted one in the busy run; in the
        established run the context has been synchronised behind the call that gave the address."""
        import torch

        class View:
            __cuda_array_interface__ = dict(shape=(count,), typestr='<i8', data=(int(ptr), False), version=2)
        src = torch.as_tensor(View(), device='cuda')
        first = (dst.ptr - dst.t.data_ptr()) // dst.t.element_size()
        words = dst.t.view(torch.int64) if dst.t.dtype != torch.int64 else dst.t
        if dst.t.dtype == torch.uint8:
            first //= 8
        words[first:first + count].copy_(src, non_blocking=True)

    def keep(self, name, a):
        self.kept[name] = np.array(a, copy=True)

    def finish(self):
        """Outputs aside, inputs poisoned again (both in stream order), one synchronisation -> results."""
        import torch
        if self.busy:
            try:
                aside = [t.clone() for t in self.outs]
                for dst, _ in self.fills:
                    if not any(dst is o for o in self.outs):
                        dst.fill_(poison_value(dst.dtype))
            finally:
                self._cm.__exit__(None, None, None)
        else:
            self.ctx.synchronize()
            aside = self.outs
        torch.cuda.synchronize()
        self._clean()
        res = {'out%d' % i: t.cpu().numpy().view(np.uint8).copy() for i, t in enumerate(aside)}
        res.update(('kept ' + k, v.view(np.uint8).reshape(-1)) for k, v in self.kept.items())
        return res

    def _clean(self):
        while self.cleanup:
            self.cleanup.pop()()

    def abort(self):
        try:
            if self.busy and self.stream is not None:
                self._cm.__exit__(None, None, None)
            else:
                self.ctx.synchronize()
        finally:
            self._clean()


def guards_intact(res, guarded):
    """Of every `out` of a run (Driver.guarded): the sentinels in front of and behind the results are untouched, and no
    result is the sentinel (never written)."""
    guard = np.float64(SENTINEL).view(np.int64)
    for name in guarded:
        w = res[name].view(np.int64)
        assert np.all(w[:_LEAD] == guard), '%s: store in front of the results' % name
        assert np.all(w[-_TAIL:] == guard), '%s: store behind the results' % name
        assert not np.any(w[_LEAD:-_TAIL] == guard), '%s: a result was not written' % name


def run_both(hip_ctx, case, name, syncs=False):
    """`case(d)` the established way, then on the busy adopted stream -> (results, results, the busy driver)."""
    out = []
    for busy_run in (False, True):
        d = Driver(hip_ctx, busy_run, name, syncs)
        try:
            case(d)
        except BaseException:
            d.abort()
            raise
        out.append(d.finish())
    return out[0], out[1], d


def assert_same(ref, got, name):
    assert ref.keys() == got.keys()
    for key in ref:
        same = ref[key].shape == got[key].shape and np.array_equal(ref[key], got[key])
        if not same:
            a, b = ref[key], got[key]
            where = np.flatnonzero(a != b) if a.shape == b.shape else []
            raise AssertionError('%s: %s differs between the synchronous run and the busy adopted stream in %d of %d bytes '
                                 '(first at byte %s)' % (name, key, len(where), a.size, where[:1]))
