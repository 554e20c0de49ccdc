"""Vectorised numpy restatement of the record encoders' contract (include/sctools_hip.h,
sct_encode / sct_encode_var), and the byte-cycling inputs that exercise it.  The tables are built
from the oracle's maps (oracle.oracle._TWO, _AMBIG, _THREE) and from nothing in the package under
test.

For a record of L bytes b_0 .. b_{L-1}:
  TwoBit    code  = sum v(b_p) << 2 (L - 1 - p), v from _TWO and 0 for every other byte
            flags = bit 0: a byte in _AMBIG, bit 1: a byte in neither map
            gc    = the positions with odd v, capped at 255
  ThreeBit  v = _THREE.get(b, 6), flags = 0, gc = the positions with odd v (capped likewise)
One limb is computed with uint64 shifts, more limbs with Python ints (object arrays).
"""

import numpy as np

from oracle import oracle as O

BASES = np.frombuffer(b"ACGTacgt", np.uint8)
IUPAC = np.frombuffer(bytes(sorted(O._AMBIG)), np.uint8)


def _tables():
    v2 = np.zeros(256, np.uint8)
    f2 = np.zeros(256, np.uint8)
    v3 = np.zeros(256, np.uint8)
    for b in range(256):
        v2[b] = O._TWO.get(b, 0)
        f2[b] = 0 if b in O._TWO else (1 if b in O._AMBIG else 2)
        v3[b] = O._THREE.get(b, 6)
    return v2, f2, v3


V2, F2, V3 = _tables()
GARBAGE = np.flatnonzero(F2 == 2).astype(np.uint8)  # the bytes in neither TwoBit map


def words_for(kind, L):
    return max(1, -(-kind * L // 64))


def flags2(recs):
    """TwoBit flags of (n, L) records: bit 0 an ambiguous byte, bit 1 a byte in neither map."""
    f = np.bitwise_or.reduce(F2[recs], axis=1) if recs.shape[1] else np.zeros(len(recs), np.uint8)
    return f.astype(np.uint8)


def encode(kind, recs, words=None):
    """(n, L) uint8 records -> (codes (n, words) uint64 little-endian limbs, gc uint8[n],
    flags uint8[n])."""
    recs = np.asarray(recs, np.uint8)
    n, L = recs.shape
    if words is None:
        words = words_for(kind, L)
    assert kind * L <= 64 * words
    v = (V2 if kind == 2 else V3)[recs]
    flags = flags2(recs) if kind == 2 else np.zeros(n, np.uint8)
    gc = np.minimum((v & 1).sum(axis=1, dtype=np.int64), 255).astype(np.uint8)
    codes = np.zeros((n, words), np.uint64)
    if words == 1:
        acc = np.zeros(n, np.uint64)
        for p in range(L):
            acc |= v[:, p].astype(np.uint64) << np.uint64(kind * (L - 1 - p))
        codes[:, 0] = acc
    else:
        acc = np.zeros(n, dtype=object)  # Python ints
        for p in range(L):
            acc = (acc << kind) | v[:, p].astype(object)
        mask = (1 << 64) - 1
        for i in range(words):
            codes[:, i] = ((acc >> (64 * i)) & mask).astype(np.uint64)
    return codes, gc, flags


def encode_var(kind, buf, starts, lens):
    """One-limb records buf[starts[r] : starts[r] + lens[r]] -> (codes uint64[n], gc, flags)."""
    buf = np.asarray(buf, np.uint8)
    starts = np.asarray(starts, np.int64)
    lens = np.asarray(lens, np.int64)
    n = starts.size
    codes, gc, flags = np.zeros(n, np.uint64), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for L in np.unique(lens).tolist():
        rows = np.flatnonzero(lens == L)
        if L == 0:
            continue
        recs = buf[starts[rows][:, None] + np.arange(L)[None, :]]
        c, g, f = encode(kind, recs, 1)
        codes[rows], gc[rows], flags[rows] = c[:, 0], g, f
    return codes, gc, flags


def ints(codes):
    """(n, words) limbs -> Python ints."""
    codes = np.asarray(codes, np.uint64).reshape(len(codes), -1)
    out = np.zeros(codes.shape[0], dtype=object)
    for i in range(codes.shape[1]):
        out |= codes[:, i].astype(object) << (64 * i)
    return out.tolist()


# ---------------------------------------------------------------- inputs
# Uniform random bytes never give a clean record, so the records are drawn from ACGTacgt and
# every second one (odd i) gets 1 to 3 bytes replaced.  With j = i // 2 + phase the first
# replacement is the byte j % 256 at position (j // 256) % L: over 256 L consecutive j every
# (byte value, position) pair occurs.  The further replacements lie at offsets from that position
# and are written first, so the first one always stands.
def substitutions(i, L, phase=0):
    """The (position, value) replacements of odd record i, in the order they are written."""
    j = i // 2 + phase
    val, pos = j % 256, (j // 256) % L
    extra = j % 3  # 0, 1 or 2 further bytes (256 and 3 are coprime: every value meets every count)
    subs = [((pos + m * (1 + j % 5)) % L, (val * 7 + 13 * m + 1) % 256) for m in range(extra, 0, -1)]
    return subs + [(pos, val)]


def records(n, L, seed, phase=0):
    """(n, L) uint8 records as described above."""
    rng = np.random.default_rng(seed)
    recs = BASES[rng.integers(0, 8, (n, L))]
    if L == 0:
        return recs
    odd = np.arange(1, n, 2)
    j = odd // 2 + phase
    val, pos, extra = j % 256, (j // 256) % L, j % 3
    for m in (2, 1):
        rows = odd[extra >= m]
        jj = j[extra >= m]
        recs[rows, (pos[extra >= m] + m * (1 + jj % 5)) % L] = (val[extra >= m] * 7 + 13 * m + 1) % 256
    recs[odd, pos] = val
    return recs


def coverage(recs, phase=0):
    """bool[L, 256]: byte value seen at the position by a first replacement of `records`."""
    n, L = recs.shape
    seen = np.zeros((L, 256), bool)
    odd = np.arange(1, n, 2)
    j = odd // 2 + phase
    val, pos = j % 256, (j // 256) % L
    assert np.array_equal(recs[odd, pos], val)  # the first replacement stands in every odd record
    seen[pos, val] = True
    return seen


def check_input(recs, phase=0, full=None):
    """The conditions every test asserts on its own input before the device sees it: clean records
    exist, flagged ones (ambiguous, invalid and both) exist, and the byte values are covered.

    full (default: n >= 2 * 256 * L): all 256 values at every position, hence at every position
    mod 4 and in every dword index k < L / 4.  A smaller batch cannot hold that many replacements
    (n / 2 first ones, fewer than 4 * 256 below n = 2048); there the n // 2 consecutive (value,
    position) pairs the generator promises are required, and the callers move `phase` from batch to
    batch so that the batches of one test together cover the table."""
    n, L = recs.shape
    flags = flags2(recs)
    assert (flags == 0).any() and (flags == 1).any() and (flags == 2).any()
    seen = coverage(recs, phase)
    if full is None:
        full = n >= 2 * 256 * L
    if full:
        assert_covered(seen)
    else:
        assert int(seen.sum()) == min(n // 2, 256 * L)
    return seen


def assert_covered(seen):
    """All 256 values at every position, hence at every position mod 4 and in every dword index
    k < L / 4 (`seen` of one batch, or the OR over the batches of one test)."""
    L = seen.shape[0]
    assert seen.all()
    for q in range(min(4, L)):
        assert seen[q::4].any(axis=0).all()
    for k in range(L // 4):
        assert seen[4 * k:4 * k + 4].any(axis=0).all()
