"""The definition of dicow_bootstrap_sums (include/dicow_hip.h) twice: in plain Python integers, and vectorised with numpy for the larger
cases (tests/test_host_bootstrap.py holds the second against the first).

    w(r, p, t) = Philox4x32-10(counter = (p >> 2, r & 0xffffffff, r >> 32, t), key = (seed & 0xffffffff, seed >> 32))[p & 3]
    resample (t = 0)   out[row][c] = sum_p table[lo_s + ((w * n_s) >> 32)][c]         s the stratum of slot p, r = first_replicate + row
    swap     (t = 1)   out[row][c] = sum_p table[p][(c + (C // 2) * (w & 1)) % C]
"""
import numpy as np

M0, M1, W0, W1, MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Random123's philox4x32 with 10 rounds: four 32-bit counter words and two key words -> four 32-bit words."""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def word(seed, r, p, t):
    r &= (1 << 64) - 1
    return philox4x32_10((p >> 2, r & MASK, r >> 32, t), (seed & MASK, (seed >> 32) & MASK))[p & 3]


def draws(n, offsets, seed, r):
    """The units that replicate r draws in resample mode, slot by slot."""
    offsets = [0, n] if offsets is None else list(offsets)
    out = []
    for s in range(len(offsets) - 1):
        lo, ns = offsets[s], offsets[s + 1] - offsets[s]
        out += [lo + ((word(seed, r, p, 0) * ns) >> 32) for p in range(lo, lo + ns)]
    return out


def sums(table, replicates, seed=0, offsets=None, mode="resample", first_replicate=0):
    """table: a list of n rows of C Python integers -> a list of `replicates` rows of C Python integers."""
    n, C = len(table), len(table[0])
    out = []
    for row in range(replicates):
        r = first_replicate + row
        acc = [0] * C
        if mode == "resample":
            for u in draws(n, offsets, seed, r):
                for c in range(C):
                    acc[c] += table[u][c]
        else:
            for p in range(n):
                b = word(seed, r, p, 1) & 1
                for c in range(C):
                    acc[c] += table[p][(c + (C // 2) * b) % C]
        out.append(acc)
    return out


def philox_np(c0, c1, c2, c3, k0, k1):
    """philox4x32_10 on uint64 arrays holding 32-bit values (broadcast against each other)."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) for c in (c0, c1, c2, c3))
    k0, k1, mask, sh = np.uint64(k0), np.uint64(k1), np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> sh) ^ c1 ^ k0, p1 & mask, (p0 >> sh) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(W0)) & mask, (k1 + np.uint64(W1)) & mask
    return c0, c1, c2, c3


def words_np(n, replicates, seed, first_replicate, t):
    """uint64 [replicates, n]: w(first_replicate + row, p, t)."""
    r = [(first_replicate + row) & ((1 << 64) - 1) for row in range(replicates)]
    rlo = np.asarray([x & MASK for x in r], np.uint64)[:, None]
    rhi = np.asarray([x >> 32 for x in r], np.uint64)[:, None]
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)[None, :]
    w = philox_np(blocks, rlo, rhi, np.uint64(t), seed & MASK, (seed >> 32) & MASK)
    return np.stack(np.broadcast_arrays(*w), axis=2).reshape(replicates, -1)[:, :n]


def sums_np(table, replicates, seed=0, offsets=None, mode="resample", first_replicate=0):
    """The same sums with numpy: table int64 [n, C] -> int64 [replicates, C] (the caller keeps n * max|table| below 2^62)."""
    table = np.asarray(table, np.int64)
    n, C = table.shape
    if replicates == 0:
        return np.zeros((0, C), np.int64)
    if mode == "resample":
        offsets = np.asarray([0, n] if offsets is None else offsets, np.int64)
        size = np.repeat(np.diff(offsets), np.diff(offsets)).astype(np.uint64)[None, :]
        first = np.repeat(offsets[:-1], np.diff(offsets))[None, :]
        u = first + ((words_np(n, replicates, seed, first_replicate, 0) * size) >> np.uint64(32)).astype(np.int64)
        return table[u].sum(axis=1)
    b = (words_np(n, replicates, seed, first_replicate, 1) & np.uint64(1)).astype(bool)[:, :, None]
    return np.where(b, np.roll(table, -(C // 2), axis=1)[None], table[None]).sum(axis=1)
