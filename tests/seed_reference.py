"""The SPECTRAL seed's contract in plain Python: what sct_allpairs_seed_rows must write, for all four
seed forms (int8 / int16 / int32 on 14-bit columns, int8 on 16-bit columns), written from the rule
and not from the kernels.

  rows          seed(z, c) = sum over the codes whose low `column_bits` bits are c of
                (-1)^popcount((code >> column_bits) & z)
  row_position  where a row of elem_bytes-wide values holds column c (the tile's register layout:
                one 16-byte chunk carries V = 16 / elem_bytes columns of one tile thread)
  stored        rows as the device holds them: column c at row_position(c), in the seed's type
  launch_shape  (walks, walks per workgroup, log2 walks per Gray-ordered block) of a slice range
"""
import numpy as np

WALK = 64              # slices per Gray walk
SEED_WALKS = 16        # walks per workgroup at most
MAX_BLOCK_BITS = 4     # walks per Gray-ordered block: <= 16
MIN_WORKGROUPS = 4096  # the int8 seeds keep at least this grid: 2^column_bits / 256 column blocks x rows
WIDE_MIN_ROWS = 64     # the int16 / int32 seeds keep at least this many workgroup rows
DTYPES = {1: np.int8, 2: np.int16, 4: np.int32}


def _parity(x):
    x = x.copy()
    for s in (16, 8, 4, 2, 1):
        x ^= x >> np.uint32(s)
    return x & np.uint32(1)


def rows_at(codes, column_bits, z):
    """[len(z)][2^column_bits] int32: the seed rows of the slices `z` (any order, any subset)."""
    codes = np.asarray(codes, dtype=np.uint64)
    z = np.asarray(z, dtype=np.uint32)
    col = (codes & np.uint64((1 << column_bits) - 1)).astype(np.int64)
    order = np.argsort(col, kind="stable")
    col = col[order]
    hi = (codes >> np.uint64(column_bits)).astype(np.uint32)[order]
    out = np.zeros((z.size, 1 << column_bits), np.int32)
    if codes.size == 0 or z.size == 0:
        return out
    sign = 1 - 2 * _parity(hi[None, :] & z[:, None]).astype(np.int32)  # [slice][code], codes by column
    first = np.flatnonzero(np.r_[True, col[1:] != col[:-1]])           # non-empty columns only
    out[:, col[first]] = np.add.reduceat(sign, first, axis=1)
    return out


def rows(codes, column_bits, z0, z1):
    """[z1 - z0][2^column_bits] int32: the seed rows of slices [z0, z1)."""
    return rows_at(codes, column_bits, np.arange(z0, z1, dtype=np.uint32))


def row_position(c, elem_bytes):
    """Position of column c (14-bit; scalar or array) in a stored row.  A 16-byte chunk holds V
    columns that differ in their low L bits; the chunk index is the column's bits 4..11 (the tile
    thread), then its bits L..3, then its bits 12 and 13.  The identity for int8."""
    V = 16 // elem_bytes
    L = V.bit_length() - 1
    return (c & (V - 1)) | (((c >> 4) & 255) << L) | (((c >> L) & (16 // V - 1)) << (L + 8)) | ((c >> 12) << 12)


def stored(ref, column_bits, elem_bytes):
    """Reference rows (int32, by column) as the device holds them."""
    assert np.abs(ref).max(initial=0) <= np.iinfo(DTYPES[elem_bytes]).max
    if elem_bytes == 1:
        return ref.astype(np.int8)
    assert column_bits == 14
    out = np.empty(ref.shape, DTYPES[elem_bytes])
    out[:, row_position(np.arange(1 << 14), elem_bytes)] = ref
    return out


def launch_shape(column_bits, elem_bytes, z0, z1):
    """(walks, per_wg, lp) of the seed launch of slices [z0, z1): the 64-slice walks the range
    touches, the walks one workgroup takes, and log2 of the walks per Gray-ordered block (int8
    seeds; the int16 / int32 seeds stride over single walks: lp = 0)."""
    walks = (z1 - (z0 & ~(WALK - 1)) + WALK - 1) // WALK
    if elem_bytes == 1:
        min_rows = MIN_WORKGROUPS // ((1 << column_bits) // 256)
        per_wg = max(1, min(SEED_WALKS, walks // min_rows))
        lp = 0
        while lp < MAX_BLOCK_BITS and (2 << lp) <= per_wg:
            lp += 1
        return walks, per_wg, lp
    return walks, max(1, min(SEED_WALKS, walks // WIDE_MIN_ROWS)), 0
