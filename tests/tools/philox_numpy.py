"""numpy restatement of the counter-based generator of the Monte-Carlo kernels (csrc/philox.hpp): Philox4x32-10 (Salmon et al., SC'11, the
constants of Random123), Random123's known-answer vectors, and the two 53-bit uniform rules include/met2_hip.h states.  Independent of the
device code: the GPU tests compare the kernels' draws with it."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)

# Random123's kat_vectors for philox4x32_10: (counter, key, output words)
KNOWN_ANSWERS = (
    ([0, 0, 0, 0], [0, 0], ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]),
)


def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays (broadcastable), key: 2 uint32 arrays -> the 4 output words (uint32 arrays)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint32) for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint32) for k in key)
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0 = (k0 + W0).astype(np.uint32)
                k1 = (k1 + W1).astype(np.uint32)
            p0 = M0 * c0.astype(np.uint64)
            p1 = M1 * c2.astype(np.uint64)
            n0 = (p1 >> np.uint64(32)).astype(np.uint32) ^ c1 ^ k0
            n2 = (p0 >> np.uint64(32)).astype(np.uint32) ^ c3 ^ k1
            c0, c1, c2, c3 = n0, p1.astype(np.uint32), n2, p0.astype(np.uint32)
    return c0, c1, c2, c3


def words(*xs):
    return ["%08x" % int(x) for x in xs]


def check_known_answers():
    for ctr, key, want in KNOWN_ANSWERS:
        assert words(*philox4x32_10(ctr, key)) == want, (ctr, key)


def u01_co(a, b, dtype=np.float64):
    """the 53-bit uniform in [0, 1) from two words: ((a >> 5) 2^26 + (b >> 6)) 2^-53 (exact in float64 and wider)"""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    return ((a >> np.uint32(5)).astype(dtype) * dtype(2.0 ** 26) + (b >> np.uint32(6)).astype(dtype)) * dtype(2.0 ** -53)


def u01_oc(a, b, dtype=np.float64):
    """the 53-bit uniform in (0, 1]: ((a >> 5) 2^26 + (b >> 6) + 1) 2^-53 (the Box-Muller radius takes its log)"""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    return ((a >> np.uint32(5)).astype(dtype) * dtype(2.0 ** 26) + (b >> np.uint32(6)).astype(dtype) + dtype(1.0)) * dtype(2.0 ** -53)


def halves(x):
    """(lo32, hi32) as uint32 arrays of 64-bit integers; Python ints in [-2^63, 2^64) are taken modulo 2^64 (a seed of -1 is 2^64 - 1)"""
    x = np.asarray([int(v) % 2 ** 64 for v in np.atleast_1d(np.asarray(x, dtype=object)).ravel()], dtype=np.uint64)
    return (x & np.uint64(0xFFFFFFFF)).astype(np.uint32), (x >> np.uint64(32)).astype(np.uint32)


def voxel_words(seed, ids, c0, stream):
    """the 4 output words at counter (c0, stream, lo32(id), hi32(id)), key (lo32(seed), hi32(seed)), broadcast over ids [n] x c0 [m] ->
    4 arrays [n, m]"""
    k0, k1 = halves(seed)
    lo, hi = halves(ids)
    c0 = np.atleast_1d(np.asarray(c0, dtype=np.uint32))
    shape = (lo.shape[0], c0.shape[0])
    ctr = [np.broadcast_to(c0[None, :], shape), np.full(shape, stream, dtype=np.uint32), np.broadcast_to(lo[:, None], shape),
           np.broadcast_to(hi[:, None], shape)]
    return philox4x32_10(ctr, (k0[0], k1[0]))
