"""Plain-Python Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) for the
device generator's known-answer test.  Checked below against the paper's published test vectors."""
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & 0xffffffff, p1 & 0xffffffff, ((p0 >> 32) ^ c3 ^ k1) & 0xffffffff, p0 & 0xffffffff
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return [c0, c1, c2, c3]


def philox4x32_10_vec(counter, key):
    """The same ten rounds over arrays of counters: `counter` four and `key` two arrays (or scalars) of 32-bit words, all
    broadcast against each other -> four uint64 arrays of 32-bit words.  Every operand is kept uint64: NumPy promotes a
    uint64 array combined with a signed integer array to float64, and a product of two 32-bit words needs all 64 bits."""
    import numpy as np
    u64 = np.uint64
    lo, s32 = u64(0xffffffff), u64(32)
    words = np.broadcast_arrays(*[np.asarray(v, dtype=u64) for v in tuple(counter) + tuple(key)])
    c0, c1, c2, c3, k0, k1 = [w.copy() for w in words]
    for _ in range(10):
        p0, p1 = u64(M0) * c0, u64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & lo, (p0 >> s32) ^ c3 ^ k1, p0 & lo
        k0, k1 = (k0 + u64(W0)) & lo, (k1 + u64(W1)) & lo
    return [c0, c1, c2, c3]


def uniform53_first(seed, stream, idx):
    """The device's 53-bit uniform from the first two words of counter `idx` of stream (seed, stream): ((r0 << 21) |
    (r1 >> 11)) 2^-53 (csrc/philox.hpp; the word a mixture draw picks its component with)."""
    import numpy as np
    u64 = np.uint64
    idx = np.asarray(idx, dtype=u64)
    lo, s32 = u64(0xffffffff), u64(32)
    seed, stream = u64(seed), u64(stream)
    r = philox4x32_10_vec((idx & lo, idx >> s32, stream & lo, stream >> s32), (seed & lo, seed >> s32))
    return ((r[0] << u64(21)) | (r[1] >> u64(11))).astype(np.float64) * 2.0 ** -53


# Random123 kat_vectors, philox4x32 10 rounds
assert philox4x32_10((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
assert philox4x32_10((0xffffffff,) * 4, (0xffffffff,) * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
assert philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
    [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
