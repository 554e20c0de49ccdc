"""CPU: tests/feature_resolve_reference.py, the contract of "resolving features"
(include/sctools_hip.h) in plain Python, against cases worked by hand and its own invariants."""

import pytest

import count_matrix_reference as M
import feature_resolve_reference as F

C, A, G, T = 1, 2, 3, 4


def umi3(*bases):
    """A ThreeBit code written first base first (the first base in the high triplet)."""
    code = 0
    for b in bases:
        code = (code << 3) | b
    return code


def counter(nw, nf, L, reads):
    """A FeatureMolecules fed {(index, feature, umi): reads}."""
    fm = M.FeatureMolecules(nw, nf, 3, L)
    for (i, f, u), r in reads.items():
        fm.update([i] * r, [u] * r, [f] * r)
    return fm


def worked_case():
    """Barcode 0, A' one base from A: feature 1 has A x 1 and A' x 3, feature 2 has A' x 3."""
    a, a2 = umi3(A, A, C), umi3(A, A, G)
    return counter(1, 3, 3, {(0, 1, a): 1, (0, 1, a2): 3, (0, 2, a2): 3}), a, a2


def test_collapse_comes_first():
    fm, a, a2 = worked_case()
    # A' ties 3 : 3 and both members drop; A stays
    assert F.answer(fm, "none") == ([1], 1, 0, 2, 6)
    assert F.resolve(F.rows_of(fm, "none"))[0] == {(0, 1, a)}
    assert F.matrix_resolved(fm, "none") == ([0, 2], [1, 2], [2, 1], [4, 3], None, [1, 0])
    # feature 1's image A' carries 4 reads and beats feature 2's 3
    for method in ("one_step", "directional"):
        assert F.answer(fm, method) == ([1], 1, 1, 0, 3)
        assert F.resolve(F.rows_of(fm, method))[0] == {(0, 1, a2)}
        assert F.matrix_resolved(fm, method) == ([0, 2], [1, 2], [2, 1], [4, 3], [1, 1], [1, 0])


@pytest.mark.parametrize("method", F.METHODS)
def test_one_kept_and_two_lost(method):
    u = umi3(G, T, C)
    fm = counter(2, 4, 3, {(1, 0, u): 5, (1, 2, u): 3, (1, 3, u): 3})
    assert F.answer(fm, method) == ([0, 1], 1, 2, 0, 6)
    assert F.matrix_resolved(fm, method)[5] == [1, 0, 0]


@pytest.mark.parametrize("method", F.METHODS)
def test_three_tied_with_one_below_the_top(method):
    u = umi3(G, T, C)
    fm = counter(2, 4, 3, {(1, 0, u): 3, (1, 2, u): 3, (1, 3, u): 1})
    assert F.answer(fm, method) == ([0, 0], 1, 0, 3, 7)
    assert F.matrix_resolved(fm, method)[5] == [0, 0, 0]


@pytest.mark.parametrize("method", F.METHODS)
def test_a_single_feature_group_keeps_its_molecule(method):
    fm = counter(2, 4, 3, {(0, 3, umi3(C, C, C)): 2, (1, 1, umi3(T, T, T)): 1})
    assert F.answer(fm, method) == ([1, 1], 0, 0, 0, 0)
    assert F.matrix_resolved(fm, method)[5] == [1, 1]


def test_fold():
    assert F.fold([]) == (0, 0, 0, 0)
    assert F.fold([4]) == (4, 1, 1, 4)
    assert F.fold([5, 3, 3]) == (5, 1, 3, 11)
    assert F.fold([3, 3, 1]) == (3, 2, 3, 7)
    assert F.fold([2, 2, 2, 1]) == (2, 2, 4, 7)


def test_raw_dict_rows():
    rows = F.rows_from_dict({(0, 1, 9): 2, (0, 0, 9): 1, (1, 0, 9): 1})
    assert rows == [(0, 0, 9, 1, 9), (0, 1, 9, 2, 9), (1, 0, 9, 1, 9)]
    assert F.resolve(rows) == ({(0, 1, 9), (1, 0, 9)}, 1, 1, 0, 1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_invariants_on_a_random_mix(seed):
    nw, nf, L = 5, 6, 6
    index, feature, umi = F.mix(seed, n=3000, nw=nw, nf=nf, L=L)
    fm = M.FeatureMolecules(nw, nf, 3, L).update(index, umi, feature)
    for method in F.METHODS:
        alone, unique, tied = F.group_kinds(F.rows_of(fm, method))
        assert alone >= 5 and unique >= 5 and tied >= 5, (method, alone, unique, tied)
        resolved, n_shared, n_lost, n_tied, dropped = F.answer(fm, method)
        indptr, _, molecules, reads, collapsed, per_entry = F.matrix_resolved(fm, method)
        assert n_shared == unique + tied
        bound = molecules if method == "none" else collapsed
        assert sum(resolved) + n_lost + n_tied == sum(bound)
        assert all(r <= b for r, b in zip(per_entry, bound))
        assert [sum(per_entry[indptr[i]:indptr[i + 1]]) for i in range(nw)] == resolved
        assert 0 < dropped < sum(reads)


@pytest.mark.parametrize("method", F.METHODS)
def test_nothing_shared_changes_nothing(method):
    nw, nf, L = 3, 4, 5
    index, feature, umi = F.mix(5, n=400, nw=nw, nf=nf, L=L, hop=0.0, err=0.0, planted=0)
    fm = M.FeatureMolecules(nw, nf, 3, L).update(index, umi, feature)
    resolved, n_shared, n_lost, n_tied, dropped = F.answer(fm, method)
    _, _, molecules, _, collapsed, per_entry = F.matrix_resolved(fm, method)
    assert (n_shared, n_lost, n_tied, dropped) == (0, 0, 0, 0)
    assert per_entry == (molecules if method == "none" else collapsed)
