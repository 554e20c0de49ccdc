"""The contract of the close-pairs pass (sct_allpairs_close_pairs, Barcodes.close_pairs), in plain
numpy: which barcodes of a set lie within ``max_d`` bases of each other.

The distance is ``oracle.pair_distances_numpy``: the number of non-zero 2-bit groups of ``a ^ b``
(TwoBit.hamming_distance, encodings.py:113-121).  Indices are positions in the input array; equal
codes (a multiset) are pairs at distance 0."""

import numpy as np

from oracle import oracle as O


def close_pairs(codes, code_bits, max_d):
    """(i, j, dist): every i < j < n with d(codes[i], codes[j]) <= max_d, rows ascending by (i, j);
    i and j int32, dist uint8.  ``code_bits`` bounds the codes (every code < 2**code_bits)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint64).reshape(-1)
    n = codes.size
    assert code_bits >= 64 or n == 0 or int(codes.max()) < 1 << code_bits
    ii, jj, dd = [], [], []
    for i in range(n - 1):
        d = O.pair_distances_numpy(codes[i], codes[i + 1:])
        hit = np.flatnonzero(d <= max_d)
        if hit.size:
            ii.append(np.full(hit.size, i, dtype=np.int32))
            jj.append((hit + (i + 1)).astype(np.int32))
            dd.append(d[hit].astype(np.uint8))
    if not ii:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.uint8)
    return np.concatenate(ii), np.concatenate(jj), np.concatenate(dd)


def neighbour_counts(codes, code_bits, max_d):
    """(n, max_d + 1) int64: [k, d] = the other positions at distance exactly d from position k
    (each pair counts at both of its ends)."""
    n = np.asarray(codes).reshape(-1).size
    i, j, dist = close_pairs(codes, code_bits, max_d)
    out = np.zeros((n, max_d + 1), dtype=np.int64)
    np.add.at(out, (i, dist), 1)
    np.add.at(out, (j, dist), 1)
    return out
