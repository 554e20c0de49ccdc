"""CPU: the swapped-molecule removal's Python restatement (tests/swapped_reference.py) on its own, on
the base case the device test uses -- the two overlapping halves of test_gpu_molecules_merge -- so the
identities the README states hold for the reference before the device is compared with it by exact
equality (tests/test_gpu_swapped.py)."""

import functools

import pytest

import count_matrix_reference as C
import swapped_reference as S
import test_gpu_molecules_merge as MM
import umi_directional_reference as UD

FRACTIONS = [(4, 5), (2, 3), (3, 5), (1, 1)]


def fed(nw, kind, L, *batches):
    ref = UD.DirectionalMolecules(nw, kind, L)
    for index, umis in batches:
        ref.update(index, umis)
    return ref


def empty_like(ref):
    if isinstance(ref, C.FeatureMolecules):
        return C.FeatureMolecules(ref.nw, ref.nf, ref.kind, ref.L)
    return UD.DirectionalMolecules(ref.nw, ref.kind, ref.L)


def cleaned(refs, num, den):
    """([the cleaned reference of every sample], [its tally]) into empty counters."""
    out = [empty_like(r) for r in refs]
    return out, [S.remove_swapped(refs, k, num, den, out[k]) for k in range(len(refs))]


def shown(ref):
    return ref.counts(), sorted(ref.mreads.items()), ref.total, list(ref.tally)


@functools.lru_cache(maxsize=None)
def base():
    """((a's reads, b's reads), (a's reference, b's reference)): ThreeBit L = 4 under 7 barcodes, the
    halves of test_gpu_molecules_merge._overlap().  227 keys are in both; at 4/5 a keeps 10 of them,
    b 18 and 199 are dropped by both, 12 of the 28 kept sit exactly at equality; at 2/3 it is 60, 60
    and 107; at 1/1 all 227 are dropped."""
    nw, kind, L, a, b, _, _, _ = MM._overlap()
    ra, rb = fed(nw, kind, L, a), fed(nw, kind, L, b)
    both = set(ra.mreads) & set(rb.mreads)
    kept_a = [k for k in both if S.keeps(ra.mreads[k], rb.mreads[k], 4, 5)]
    kept_b = [k for k in both if S.keeps(rb.mreads[k], ra.mreads[k], 4, 5)]
    equal = [k for k in both if 5 * max(ra.mreads[k], rb.mreads[k]) == 4 * (ra.mreads[k] + rb.mreads[k])]
    assert len(kept_a) >= 10 and len(kept_b) >= 10 and len(both) - len(kept_a) - len(kept_b) >= 150
    assert len(equal) >= 10
    assert sum(ra.mreads[k] == rb.mreads[k] for k in both) >= 50
    return (a, b), (ra, rb)


def test_the_base_case_is_what_the_device_test_counts_on():
    _, (ra, rb) = base()
    both = set(ra.mreads) & set(rb.mreads)
    assert len(both) == 227
    for (num, den), want in zip(FRACTIONS[:2] + FRACTIONS[3:], [(10, 18, 199), (60, 60, 107), (0, 0, 227)]):
        out, tally = cleaned([ra, rb], num, den)
        in_a, in_b = both & set(out[0].mreads), both & set(out[1].mreads)
        assert (len(in_a), len(in_b), len(both - in_a - in_b)) == want
        assert tally[0][:2] == [227, 227 - len(in_a)] and tally[1][:2] == [227, 227 - len(in_b)]


def test_reads_are_kept_or_tallied_and_a_key_has_one_owner():
    _, refs = base()
    for num, den in FRACTIONS:
        before = [shown(r) for r in refs]
        out, tally = cleaned(list(refs), num, den)
        assert [shown(r) for r in refs] == before  # no sample is changed
        assert sum(sum(o.reads) for o in out) + sum(t[2] for t in tally) == sum(sum(r.reads) for r in refs)
        assert not set(out[0].mreads) & set(out[1].mreads)
        for o, r, t in zip(out, refs, tally):
            assert o.tally == r.tally and o.total == sum(o.reads) + sum(o.tally)
            assert len(o.mreads) == len(r.mreads) - t[1] and sum(o.molecules) == len(o.mreads)
            assert all(o.mreads[k] == r.mreads[k] for k in o.mreads)  # a kept molecule keeps all its reads
            assert o.seen == set(o.mreads)


def test_a_stricter_fraction_keeps_a_subset():
    _, refs = base()
    kept = [set(cleaned(list(refs), num, den)[0][0].mreads) for num, den in ((3, 5), (2, 3), (4, 5), (1, 1))]
    assert all(b < a for a, b in zip(kept, kept[1:]))
    unshared = set(refs[0].mreads) - set(refs[1].mreads)
    assert kept[-1] == unshared  # num == den keeps the unshared molecules only


def test_one_sample_is_a_copy_and_the_same_call_twice_adds_reads_only():
    _, (ra, rb) = base()
    alone = empty_like(ra)
    assert S.remove_swapped([ra], 0, 4, 5, alone) == [0, 0, 0]
    assert shown(alone) == shown(ra)
    once, twice = empty_like(ra), empty_like(ra)
    S.remove_swapped([ra, rb], 0, 4, 5, once)
    assert S.remove_swapped([ra, rb], 0, 4, 5, twice) == S.remove_swapped([ra, rb], 0, 4, 5, twice)
    assert twice.molecules == once.molecules and twice.reads == [2 * x for x in once.reads]
    assert twice.total == 2 * once.total and twice.tally == [2 * x for x in once.tally]
    assert all(twice.mreads[k] == 2 * r for k, r in once.mreads.items())


def test_into_a_counter_that_holds_overlapping_molecules():
    (a, b), (ra, rb) = base()
    nw, kind, L = ra.nw, ra.kind, ra.L
    into = fed(nw, kind, L, b)  # holds every key b has: a's kept shared keys are there already
    clean = empty_like(ra)
    S.remove_swapped([ra, rb], 0, 4, 5, clean)
    S.remove_swapped([ra, rb], 0, 4, 5, into)
    assert set(clean.mreads) & set(rb.mreads)
    assert set(into.mreads) == set(rb.mreads) | set(clean.mreads)
    assert all(into.mreads[k] == rb.mreads.get(k, 0) + clean.mreads.get(k, 0) for k in into.mreads)
    assert sum(into.molecules) == len(into.mreads) and into.total == rb.total + clean.total


def test_a_feature_is_part_of_the_molecule():
    """The same (index, UMI) under feature 1 in one sample and feature 2 in the other is not shared;
    under the same feature it is."""
    umi = MM.umi3(MM.A, MM.C, MM.G, MM.T)
    x = C.FeatureMolecules(7, 5, 3, 4).update([3] * 9 + [3], [umi] * 10, [1] * 9 + [4])
    y = C.FeatureMolecules(7, 5, 3, 4).update([3, 3], [umi, umi], [2, 4])
    out, tally = cleaned([x, y], 4, 5)
    assert tally == [[1, 1, 1], [1, 1, 1]]  # (3, 4, umi) is shared at 1 : 1 and dropped by both
    assert set(out[0].mreads) == {(3, 1, umi)} and set(out[1].mreads) == {(3, 2, umi)}
    assert out[0].mreads[(3, 1, umi)] == 9


def test_bad_parameters_are_refused():
    _, (ra, rb) = base()
    for s, k, num, den in ((2, 2, 4, 5), (2, -1, 4, 5), (2, 0, 1, 2), (2, 0, 0, 1), (2, 0, 5, 4),
                           (2, 0, 2 ** 32 + 1, 2 ** 32 + 1)):
        with pytest.raises(ValueError):
            S.remove_swapped([ra, rb][:s], k, num, den, empty_like(ra))
    with pytest.raises(ValueError):
        S.remove_swapped([ra] * 17, 0, 4, 5, empty_like(ra))
