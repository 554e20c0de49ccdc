"""Code families that drive the SPECTRAL tile kernels to the bounds their comments document.

For a column width `bits` (14 or 16: the low bits of a code, the rest is its slice part) every
column c in [0, 2^bits) holds one distinct code m times:

    saturating     c | (parity(mask & c) ^ neg) * e << bits
    random_sign    c | h_c << bits,   h_c drawn from the span of three slice bits

In slice z the seed of column c is m (-1)^<code >> bits, z>: all +m (-m: neg) in the half of the
slices with <e, z> even and m chi_mask(c) (-m chi_mask(c)) in the other half, so with m = 127
stage 1 of both tile kernels reaches +-64 * 127 and the plane sums four times that; random_sign
makes every stage-1 output m * (a sum of 64 signs).  Neither family knows which column bits the
kernels treat as stage 1, stage 2 or planes.

The reference of a family is the C oracle on its 2^bits distinct codes (`family_hist`): two
different distinct codes make m^2 pairs at their distance, one distinct code m (m - 1) / 2 pairs
at distance 0."""
import numpy as np

from oracle import oracle as O


def parity(x):
    x = np.asarray(x, dtype=np.uint64).copy()
    for s in (32, 16, 8, 4, 2, 1):
        x ^= x >> np.uint64(s)
    return x & np.uint64(1)


def saturating_distinct(bits, mask, e, neg=False):
    c = np.arange(1 << bits, dtype=np.uint64)
    p = parity(c & np.uint64(mask)) ^ np.uint64(1 if neg else 0)
    return c | ((p * np.uint64(e)) << np.uint64(bits))


def slice_span(bits):
    """The eight slice patterns spanned by the lowest, a middle and the highest slice bit."""
    hb = 32 - bits
    gens = (1, 1 << (hb // 2), 1 << (hb - 1))
    return np.array([sum(g for k, g in enumerate(gens) if (i >> k) & 1) for i in range(8)], dtype=np.uint64)


def random_sign_distinct(bits, seed):
    rng = np.random.default_rng(seed)
    h = slice_span(bits)[rng.integers(0, 8, 1 << bits)]
    return np.arange(1 << bits, dtype=np.uint64) | (h << np.uint64(bits))


def expand(distinct, m, shuffle_seed=None):
    """Each distinct code m times: sorted (one run of m per code), or shuffled."""
    codes = np.repeat(distinct, m)
    if shuffle_seed is not None:
        np.random.default_rng(shuffle_seed).shuffle(codes)
    return codes


def family_hist(distinct, m):
    """17-bin histogram of the multiset `distinct` x m, from the C oracle on `distinct` alone."""
    ref = O.c_hist_rows(distinct)[:17].astype(object) * (m * m)
    ref[0] += distinct.size * (m * (m - 1) // 2)
    return [int(v) for v in ref]
