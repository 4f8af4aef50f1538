"""The scratch-assay example model (elfi/examples/scratch_assay.py: the cell-motility model of Johnston et al. 2014 with the
summaries of Price et al. 2018) stated in NumPy, for csrc/scratch_assay.hip.

The state is a binary grid of nrows x ncols cells, at most MAX_CELLS of them.  With n_iter = int(obs_period / tau), obs_every =
int(obs_interval / tau) and n_obs = int(n_iter / obs_every) (`shape`), iteration t = 0 .. n_iter - 1 runs

  1. num_cells = the cell count; the list = the occupied cells in row-major order (np.where).
  2. a full grid: nothing happens, no draw is consumed.
  3. motility: slots k = 0 .. num_cells - 1 have a candidate C[k] in [0, num_cells), a uniform P[k] and a direction M[k];
     the slots with P[k] < pm are events, in slot order.  The event's cell is list[C[k]]; M: 0 row + 1, 1 row - 1, 2 col + 1,
     3 col - 1, clamped to the grid.  An empty target: the cell moves there and list[C[k]] is the target.
  4. proliferation: fresh C, P, M over the same num_cells slots against pp, on the list as motility left it (a cell born here
     is in no list before the next iteration); the clamped target is set to 1 whatever it was.
  5. (t + 1) % obs_every == 0: the grid is frame (t + 1) / obs_every; frame 0 is the initial grid.

The summaries are ds[j] = the number of cells that differ between frames j and j + 1, j = 0 .. n_obs - 1, then the cell count of
frame n_obs: n_obs + 1 integer-valued doubles.  `P < pm` is evaluated as it stands: a NaN selects nothing, values outside [0, 1]
are legal, no parameter value is invalid.  `events` counts the slots selected, (motility, proliferation).

Draws.  Given form: C int32, P float64, M uint8, each (n, n_iter, 2, cells); row (t, f) feeds phase f (0 motility, 1
proliferation) of iteration t, entries at k >= num_cells are never read.  Every entry READ is checked: a C[k] outside [0,
num_cells) or an M[k] above 3 ends the simulation with status BAD_DRAW, NaN summaries, empty frames and zero event counts.
Drawn form: slot k of phase f of iteration t of simulation g is ONE Philox4x32-10 call of key `seed`, counter words
(((2 t + f) << 10) | k, g, stream low, stream high): C = (w0 num_cells) >> 32, P = ((w1 << 21) | (w2 >> 11)) 2^-53, M = w3 >> 30.
The direction is keyed by the slot, not by the order of the events.  (RandomState.choice rejects to be exactly uniform; the
multiply-high candidate is biased by at most num_cells / 2^32 < 2.4e-7.)

`from_random_state` consumes a RandomState in the reference's own order -- choice(num_cells, size), uniform(size), then
choice(4) per event -- and hands back the slot-keyed C, P, M it consumed (each direction at the slot of its event), so that
`simulate` on them is the reference's run.
"""
import numpy as np

import philox_ref

MAX_CELLS = 1024
OK, BAD_DRAW = 0, 1
MOVES = ((1, 0), (-1, 0), (0, 1), (0, -1))


def shape(obs_period=12, obs_interval=1 / 12, tau=1 / 24):
    """(n_iter, obs_every, n_obs) exactly as scratch_assay.py:73-75 computes them."""
    n_iter = int(obs_period / tau)
    obs_every = int(obs_interval / tau)
    return n_iter, obs_every, int(n_iter / obs_every)


def magic(ncols):
    """m with (pos m) >> 20 == pos // ncols for every 0 <= pos < 1024, 1 <= ncols <= 1024: the kernel's row of a cell."""
    return (1 << 20) // ncols + 1


class _BadDraw(Exception):
    pass


class _Given:
    """the draws of one simulation as arrays (n_iter, 2, cells)"""

    def __init__(self, C, P, M):
        self.C, self.P, self.M = C, P, M

    def phase(self, t, f, nc):
        C, M = self.C[t, f, :nc], self.M[t, f, :nc]
        if np.any((C < 0) | (C >= nc)) or np.any(M > 3):
            raise _BadDraw
        return C, self.P[t, f, :nc]

    def direction(self, t, f, k):
        return int(self.M[t, f, k])


class _FromState:
    """a RandomState in the reference's call order; records what it hands out"""

    def __init__(self, rs, n_iter, cells):
        self.rs = rs
        self.C = np.zeros((n_iter, 2, cells), dtype=np.int32)
        self.P = np.zeros((n_iter, 2, cells))
        self.M = np.zeros((n_iter, 2, cells), dtype=np.uint8)

    def phase(self, t, f, nc):
        self.C[t, f, :nc] = self.rs.choice(nc, size=nc)
        self.P[t, f, :nc] = self.rs.uniform(size=nc)
        return self.C[t, f, :nc], self.P[t, f, :nc]

    def direction(self, t, f, k):
        self.M[t, f, k] = self.rs.choice(4)
        return int(self.M[t, f, k])


def philox_words(seed, stream, g, t, f, k):
    """the four words of slot k (array) of phase f of iteration t of simulation g"""
    u64 = np.uint64
    lo = 0xffffffff
    w0 = ((2 * int(t) + int(f)) << 10) | np.asarray(k, dtype=u64)
    return philox_ref.philox4x32_10_vec((w0, int(g) & lo, int(stream) & lo, int(stream) >> 32), (int(seed) & lo, int(seed) >> 32))


def philox_phase(seed, stream, g, t, f, nc):
    """C int32, P float64, M uint8 of slots 0 .. nc - 1"""
    u64 = np.uint64
    w = philox_words(seed, stream, g, t, f, np.arange(nc, dtype=u64))
    C = ((w[0] * u64(nc)) >> u64(32)).astype(np.int32)
    P = ((w[1] << u64(21)) | (w[2] >> u64(11))).astype(np.float64) * 2.0 ** -53
    return C, P, (w[3] >> u64(30)).astype(np.uint8)


class _Philox:
    def __init__(self, seed, stream, g, n_iter):
        self.key = (seed, stream, g)
        self.nc = np.zeros((n_iter, 2), dtype=np.int32)

    def phase(self, t, f, nc):
        self.nc[t, f] = nc
        C, P, self.M = philox_phase(*self.key, t, f, nc)
        return C, P

    def direction(self, t, f, k):
        return int(self.M[k])


def _one(pm, pp, init, n_iter, obs_every, source):
    nrows, ncols = init.shape
    cells = nrows * ncols
    n_obs = n_iter // obs_every
    grid = [int(v != 0) for v in init.reshape(-1)]
    frames = np.ones((n_obs + 1, cells), dtype=np.uint8)
    frames[0] = grid
    events = [0, 0]
    try:
        for t in range(n_iter):
            cell_list = [i for i, v in enumerate(grid) if v]
            nc = len(cell_list)
            if nc != cells:
                for f, thr in ((0, pm), (1, pp)):
                    C, P = source.phase(t, f, nc)
                    for k in np.flatnonzero(P < thr):
                        pos = cell_list[C[k]]
                        dr, dc = MOVES[source.direction(t, f, k)]
                        r, c = min(max(pos // ncols + dr, 0), nrows - 1), min(max(pos % ncols + dc, 0), ncols - 1)
                        tgt = r * ncols + c
                        if f == 1:
                            grid[tgt] = 1
                        elif not grid[tgt]:
                            grid[pos], grid[tgt] = 0, 1
                            cell_list[C[k]] = tgt
                        events[f] += 1
            if (t + 1) % obs_every == 0:
                frames[(t + 1) // obs_every] = grid
    except _BadDraw:
        return np.full(n_obs + 1, np.nan), np.zeros((nrows, ncols, n_obs + 1), dtype=np.uint8), [0, 0], BAD_DRAW
    fr = frames.astype(np.int64)
    S = np.concatenate([np.abs(fr[:-1] - fr[1:]).sum(axis=1), [fr[-1].sum()]]).astype(np.float64)
    return S, frames.reshape(n_obs + 1, nrows, ncols).transpose(1, 2, 0), events, OK


def _batch(pm, pp, init, n_iter, obs_every, sources):
    n = len(sources)
    pm, pp = np.broadcast_to(np.asarray(pm, dtype=np.float64), (n,)), np.broadcast_to(np.asarray(pp, dtype=np.float64), (n,))
    out = [_one(float(pm[i]), float(pp[i]), np.asarray(init), n_iter, obs_every, sources[i]) for i in range(n)]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out], dtype=np.int64),
            np.array([o[3] for o in out], dtype=np.int32))


def simulate(pm, pp, init, C, P, M, n_iter, obs_every):
    """The given form: C, P, M (n, n_iter, 2, cells) -> S (n, n_obs + 1), frames (n, nrows, ncols, n_obs + 1) uint8 in the
    reference's layout, events (n, 2) int64, status (n) int32."""
    return _batch(pm, pp, init, n_iter, obs_every, [_Given(C[i], P[i], M[i]) for i in range(len(C))])


def from_random_state(pm, pp, init, rs, n_iter, obs_every):
    """ONE simulation (scalars pm, pp) that consumes `rs` as cell_sim does -> S (n_obs + 1), frames (nrows, ncols, n_obs + 1),
    events (2), and the draws consumed (C, P, M), each (n_iter, 2, cells), zero where nothing was drawn."""
    init = np.asarray(init)
    src = _FromState(rs, n_iter, init.size)
    S, frames, events, _ = _one(float(pm), float(pp), init, n_iter, obs_every, src)
    return S, frames, np.array(events, dtype=np.int64), (src.C, src.P, src.M)


def simulate_philox(pm, pp, init, n_iter, obs_every, seed, stream, first, n):
    """The drawn form of simulations first .. first + n - 1 -> S, frames, events, status as `simulate`, and num_cells (n,
    n_iter, 2) int32: the slots each phase drew (0 where the grid was full)."""
    sources = [_Philox(seed, stream, first + i, n_iter) for i in range(n)]
    out = _batch(pm, pp, init, n_iter, obs_every, sources)
    return out + (np.stack([s.nc for s in sources]),)


def philox_draws(seed, stream, first, num_cells, cells):
    """C, P, M (n, n_iter, 2, cells) of the drawn form for num_cells (n, n_iter, 2) slots per row, zero past them: what
    elfihip_assay_draws writes, and what the given form takes."""
    num_cells = np.asarray(num_cells)
    n, n_iter = num_cells.shape[:2]
    C = np.zeros((n, n_iter, 2, cells), dtype=np.int32)
    P = np.zeros((n, n_iter, 2, cells))
    M = np.zeros((n, n_iter, 2, cells), dtype=np.uint8)
    for i in range(n):
        for t in range(n_iter):
            for f in range(2):
                nc = int(num_cells[i, t, f])
                if nc:
                    C[i, t, f, :nc], P[i, t, f, :nc], M[i, t, f, :nc] = philox_phase(seed, stream, first + i, t, f, nc)
    return C, P, M


def summaries(frames):
    """cell_summaries of frames (n, nrows, ncols, n_obs + 1)"""
    x = np.asarray(frames).astype(np.float64)
    ds = np.sum(np.abs(x[:, :, :, :-1] - x[:, :, :, 1:]), axis=(1, 2))
    return np.concatenate((ds, np.sum(x[:, :, :, -1], axis=(1, 2))[:, None]), axis=1)


def pack_frames(frames):
    """frames (n, nrows, ncols, n_obs + 1) -> (n, n_obs + 1, 32) uint32, cell c = row ncols + col at bit c % 32 of word c // 32:
    the device's layout"""
    fr = np.asarray(frames)
    n, nrows, ncols, nf = fr.shape
    bits = np.zeros((n, nf, MAX_CELLS), dtype=np.uint8)
    bits[:, :, :nrows * ncols] = fr.transpose(0, 3, 1, 2).reshape(n, nf, -1)
    return np.packbits(bits, axis=2, bitorder='little').view('<u4')


def moments(S):
    """the five statistics of the distribution test of rows S (n, n_obs + 1): final count, sum of ds, ds[0], ds[n_obs // 2 - 1],
    ds[n_obs - 1]"""
    S = np.asarray(S)
    n_obs = S.shape[1] - 1
    return np.column_stack([S[:, -1], S[:, :-1].sum(axis=1), S[:, 0], S[:, n_obs // 2 - 1], S[:, n_obs - 1]])
