"""The read downsampling's contract (include/sctools_hip.h, "downsampling reads") restated in plain
Python: the draw written with Python integers masked to 64 bits, thin as a loop over the reads, and
downsample as a walk over a reference counter's dict of reads per molecule -- a
umi_collapse_reference.CountedMolecules (or its directional subclass) or a
count_matrix_reference.FeatureMolecules.  The device counter, the draw header and the Python class
are compared with this module by exact equality."""

import bisect

import count_matrix_reference as C
import molecules_reference as R

MASK = 2 ** 64 - 1
G = 0x9e3779b97f4a7c15
KEEP_ALL = 2 ** 32
MAX_POINTS = 64


def mix64(x):
    """murmur3's finaliser (sctools_amd/csrc/mix64.h), modulo 2^64."""
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & MASK
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & MASK
    x ^= x >> 33
    return x


def stream(seed, key):
    return mix64(key ^ mix64(seed ^ G))


def draw(seed, key, j):
    """The draw of read j = 0, 1, ... of the molecule `key`: below 2^32."""
    return mix64((stream(seed, key) + (j + 1) * G) & MASK) >> 32


def draws(seed, key, r):
    s = stream(seed, key)
    return [mix64((s + (j + 1) * G) & MASK) >> 32 for j in range(r)]


def thin(seed, key, r, threshold):
    """The reads j < r kept at `threshold`: those whose draw lies below it."""
    return sum(d < threshold for d in draws(seed, key, r))


def tally_key(k):
    """The key of tally k (0 no match, 1 ambiguous, 2 bad UMI, 3 no feature): no molecule has it."""
    return 2 ** 63 | k


def thin_tally(seed, k, n, threshold):
    return thin(seed, tally_key(k), n, threshold)


def bucket(d, thresholds):
    """The first t with d < thresholds[t] (ascending), else len(thresholds)."""
    for t, threshold in enumerate(thresholds):
        if d < threshold:
            return t
    return len(thresholds)


def thresholds_ok(thresholds):
    k = len(thresholds)
    return (1 <= k <= MAX_POINTS and all(0 <= t <= KEEP_ALL for t in thresholds)
            and all(a <= b for a, b in zip(thresholds, thresholds[1:])))


def downsample_threshold(fraction):
    if not 0 <= fraction <= 1:
        raise ValueError("fraction outside [0, 1]")
    return int(round(fraction * 2 ** 32))


def molecule_key(ref, k):
    """The 63-bit key of an entry of ref.mreads: (index, umi), or (index, feature, umi)."""
    if len(k) == 3:
        return C.key(k[0], k[1], k[2], ref.nf, ref.kind, ref.L)
    return R.key(k[0], k[1], ref.kind, ref.L)


def downsample(src, threshold, seed, into):
    """`into` (a reference counter of src's class and parameters) after it took the thinned src: what
    sct_molecules_downsample(into, src, threshold, seed) leaves.  Returns into; src is not changed."""
    if not 0 <= threshold <= KEEP_ALL:
        raise ValueError("threshold outside [0, 2^32]")
    kept = 0
    for k, r in src.mreads.items():
        m = thin(seed, molecule_key(src, k), r, threshold)
        if m == 0:
            continue
        if k not in into.mreads:
            into.mreads[k] = 0
            into.molecules[k[0]] += 1
            if hasattr(into, "seen"):
                into.seen.add(k)
        into.mreads[k] += m
        into.reads[k[0]] += m
        kept += m
    for t, n in enumerate(src.tally):
        m = thin_tally(seed, t, n, threshold)
        into.tally[t] += m
        kept += m
    into.total += kept
    return into


def curve(src, thresholds, seed):
    """(reads[k], molecules[k]) over src's stored molecules: the reads kept at thresholds[t] and the
    molecules that keep any.  Written with sorted draws, not with the buckets."""
    if not thresholds_ok(thresholds):
        raise ValueError("thresholds: 1 to 64, ascending, none above 2^32")
    reads, molecules = [0] * len(thresholds), [0] * len(thresholds)
    for k, r in src.mreads.items():
        ds = sorted(draws(seed, molecule_key(src, k), r))
        for t, threshold in enumerate(thresholds):
            m = bisect.bisect_left(ds, threshold)
            reads[t] += m
            molecules[t] += m > 0
    return reads, molecules
