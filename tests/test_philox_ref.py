"""The vectorised Philox4x32-10 of tests/philox_ref.py (the model the mixture-draw tests select components with) against
the scalar function and Random123's published vectors.  No GPU."""
import numpy as np

import philox_ref

KAT = [((0, 0, 0, 0), (0, 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]


def test_vectorised_philox_known_answers():
    ctr = [np.array([k[0][j] for k in KAT], dtype=np.uint64) for j in range(4)]
    key = [np.array([k[1][j] for k in KAT], dtype=np.uint64) for j in range(2)]
    out = philox_ref.philox4x32_10_vec(ctr, key)
    assert all(o.dtype == np.uint64 for o in out)
    for i, (_, _, want) in enumerate(KAT):
        assert [int(o[i]) for o in out] == want
    # one vector at a time, as scalars
    for c, k, want in KAT:
        assert [int(o) for o in philox_ref.philox4x32_10_vec(c, k)] == want


def test_vectorised_philox_equals_the_scalar_function():
    rs = np.random.RandomState(0)
    words = rs.randint(0, 2 ** 32, (1000, 6), dtype=np.uint64)
    words[:8, :] = np.array([0, 1, 0x7fffffff, 0x80000000, 0xfffffffe, 0xffffffff, 2, 3], dtype=np.uint64)[:, None]
    out = philox_ref.philox4x32_10_vec(list(words[:, :4].T), list(words[:, 4:].T))
    for i in range(len(words)):
        w = [int(v) for v in words[i]]
        assert [int(o[i]) for o in out] == philox_ref.philox4x32_10(w[:4], w[4:]), w
    # a key shared by all counters broadcasts
    shared = philox_ref.philox4x32_10_vec(list(words[:, :4].T), (5, 0xfffffff0))
    for i in (0, 5, 999):
        assert [int(o[i]) for o in shared] == philox_ref.philox4x32_10([int(v) for v in words[i, :4]], (5, 0xfffffff0))


def test_uniform53_uses_the_high_words_of_seed_stream_and_index():
    seed, stream = (0x1234 << 32) | 0x9abcdef1, (7 << 32) | 5
    idx = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, (3 << 32) | 9], dtype=np.uint64)
    u = philox_ref.uniform53_first(seed, stream, idx)
    assert u.dtype == np.float64 and np.all((u >= 0) & (u < 1))
    for i, e in enumerate(idx):
        e = int(e)
        r = philox_ref.philox4x32_10((e & 0xffffffff, e >> 32, stream & 0xffffffff, stream >> 32),
                                     (seed & 0xffffffff, seed >> 32))
        assert u[i] == ((r[0] << 21) | (r[1] >> 11)) / 2.0 ** 53
