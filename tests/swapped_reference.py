"""The swapped-molecule removal's contract (include/sctools_hip.h, "removing swapped molecules")
restated in plain Python: the judgement with Python integers, which never wrap, and the removal as a
walk over reference counters' dicts of reads per molecule -- umi_collapse_reference.CountedMolecules
(or its directional subclass) or count_matrix_reference.FeatureMolecules.  The device counter, the
judgement header and the Python function are compared with this module by exact equality."""

TOP = 2 ** 64 - 1
MAX_SAMPLES = 16
MAX_DEN = 2 ** 32


def add_sat(a, b):
    """a + b, saturating at 2^64 - 1."""
    return min(a + b, TOP)


def keeps(r, others, num, den):
    """Whether the sample with r reads of a molecule keeps it against `others` reads elsewhere:
    r / (r + others) >= num / den, without a division."""
    return r * (den - num) >= num * others


def params_ok(s, num, den):
    return 1 <= s <= MAX_SAMPLES and 1 <= num <= den <= MAX_DEN and 2 * num > den


def others(refs, k, key):
    """The reads of `key` in every sample but k, as a saturating sum."""
    total = 0
    for t, ref in enumerate(refs):
        if t != k:
            total = add_sat(total, ref.mreads.get(key, 0))
    return total


def remove_swapped(refs, k, num, den, into):
    """`into` (a reference counter of the samples' class and parameters) after it took the kept
    molecules of refs[k]: what sct_molecules_swapped(refs, s, k, into, num, den) leaves.  Returns the
    tally [shared, removed, removed reads]; no sample is changed."""
    if not params_ok(len(refs), num, den):
        raise ValueError("1 <= s <= 16, 1 <= num <= den <= 2^32 and 2 * num > den")
    if not 0 <= k < len(refs):
        raise ValueError("k outside [0, s)")
    src = refs[k]
    shared = removed = removed_reads = kept_reads = 0
    for key, r in src.mreads.items():
        elsewhere = others(refs, k, key)
        shared += elsewhere > 0
        if not keeps(r, elsewhere, num, den):
            removed += 1
            removed_reads += r
            continue
        if key not in into.mreads:
            into.mreads[key] = 0
            into.molecules[key[0]] += 1
            if hasattr(into, "seen"):
                into.seen.add(key)
        into.mreads[key] += r
        into.reads[key[0]] += r
        kept_reads += r
    for t, n in enumerate(src.tally):
        into.tally[t] += n
    into.total += kept_reads + sum(src.tally)
    return [shared, removed, removed_reads]
