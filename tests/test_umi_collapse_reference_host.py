"""CPU: the hand cases of the UMI collapse contract (include/sctools_hip.h, "collapsing UMIs one base
apart") on tests/umi_collapse_reference.py, the reference the device counter is compared with."""

import umi_collapse_reference as U

C, A, G, T, N = 1, 2, 3, 4, 6  # ThreeBit triplets


def umi3(*bases):
    """A ThreeBit code written first base first (the first base in the high triplet)."""
    code = 0
    for b in bases:
        code = (code << 3) | b
    return code


def _fed(nw, kind, L, molecules):
    """A reference counter fed `reads` reads of every (index, umi, reads)."""
    ref = U.CountedMolecules(nw, kind, L)
    for i, u, r in molecules:
        ref.update([i] * r, [u] * r)
    return ref


def test_chain_counts_images_not_roots():
    """AA x 1, AC x 2, GC x 5: AA -> AC -> GC.  Two images (AC, GC), one root, two corrected."""
    AA, AC, GC = umi3(A, A), umi3(A, C), umi3(G, C)
    ref = _fed(1, 3, 2, [(0, AA, 1), (0, AC, 2), (0, GC, 5)])
    assert (ref.parent(0, AA), ref.parent(0, AC), ref.parent(0, GC)) == (AC, GC, GC)
    assert ref.collapse() == ([2], 2)
    assert ref.roots() == [1] and ref.molecules == [3] and ref.reads == [8]
    assert ref.pairs_counted() == sorted([(0, AC, 2, GC), (0, AA, 1, AC), (0, GC, 5, GC)])
    assert ref.saturation() == 1 - 3 / 8 and ref.saturation_collapsed() == 1 - 2 / 8


def test_equal_reads_tie_goes_to_the_larger_code():
    """AA x 1 between CA x 3 and TA x 3 goes to TA (T = 4 > C = 1).  GG x 1 between GC x 3 and GA x 3
    goes to GA: by code A = 2 > C = 1, where ASCII order ('C' > 'A') would pick GC."""
    ref = _fed(1, 3, 2, [(0, umi3(A, A), 1), (0, umi3(C, A), 3), (0, umi3(T, A), 3)])
    assert ref.parent(0, umi3(A, A)) == umi3(T, A)
    ref = _fed(1, 3, 2, [(0, umi3(G, G), 1), (0, umi3(G, C), 3), (0, umi3(G, A), 3)])
    assert ref.parent(0, umi3(G, G)) == umi3(G, A)  # by code A 2 > C 1; by ASCII 'C' > 'A'
    assert U.support_less(3, 5, 3, 6) and not U.support_less(3, 6, 3, 5) and not U.support_less(3, 5, 3, 5)
    assert U.support_less(2, 99, 3, 1) and not U.support_less(3, 1, 2, 99)


def test_two_equal_neighbours_exactly_one_moves():
    AC, AG = umi3(A, C), umi3(A, G)
    ref = _fed(1, 3, 2, [(0, AC, 4), (0, AG, 4)])
    assert ref.parent(0, AC) == AG and ref.parent(0, AG) == AG
    assert ref.collapse() == ([1], 1)


def test_length_one_all_four_are_mutual_neighbours():
    ref = _fed(2, 3, 1, [(1, C, 2), (1, A, 7), (1, G, 7), (1, T, 1)])
    assert sorted(U.neighbours(C, 3, 1)) == [A, G, T]
    assert [ref.parent(1, u) for u in (C, A, G, T)] == [G, G, G, G]
    assert ref.collapse() == ([0, 1], 3)
    two = _fed(1, 2, 1, [(0, 0, 1), (0, 3, 1)])  # TwoBit: digit 0 is a base like any other
    assert sorted(U.neighbours(0, 2, 1)) == [1, 2, 3]
    assert two.parent(0, 0) == 3 and two.collapse() == ([1], 1)


def test_same_umi_under_two_barcodes_never_merges():
    AA, AC = umi3(A, A), umi3(A, C)
    ref = _fed(3, 3, 2, [(0, AA, 1), (2, AC, 9), (1, AA, 1), (1, AA, 1)])
    assert ref.parent(0, AA) == AA and ref.parent(2, AC) == AC and ref.parent(1, AA) == AA
    assert ref.collapse() == ([1, 1, 1], 0)
    assert ref.reads == [1, 2, 9]


def test_a_threebit_neighbour_is_never_n_or_invalid():
    for code in (umi3(C, A, G, T), umi3(T, T, T, T), umi3(C, C, C, C)):
        nbs = U.neighbours(code, 3, 4)
        assert len(nbs) == len(set(nbs)) == 12 and code not in nbs
        for v in nbs:
            assert all(d in (1, 2, 3, 4) for d in U.digits(v, 3, 4))
            assert sum(a != b for a, b in zip(U.digits(v, 3, 4), U.digits(code, 3, 4))) == 1
    # a stored UMI with N is impossible (rule 4), and an N read never becomes anyone's neighbour
    ref = _fed(1, 3, 2, [(0, umi3(A, A), 1), (0, umi3(A, N), 50)])
    assert ref.tally[2] == 50 and ref.collapse() == ([1], 0)
