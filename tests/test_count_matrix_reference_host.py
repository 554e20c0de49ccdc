"""CPU: tests/count_matrix_reference.py, the feature counter's contract in plain Python, against cases
worked by hand (include/sctools_hip.h, "counting molecules per feature")."""

import pytest

import count_matrix_reference as M

C, A, G, T, N = 1, 2, 3, 4, 6


def umi3(*bases):
    """A ThreeBit code written first base first (the first base in the high triplet)."""
    code = 0
    for b in bases:
        code = (code << 3) | b
    return code


def test_the_worked_example():
    """nw = 3, nf = 2, ThreeBit L = 2: seven reads that meet every rule."""
    AA, AC, bad = umi3(A, A), umi3(A, C), umi3(A, N)
    ref = M.FeatureMolecules(3, 2, 3, 2)
    ref.update([0, 0, 0, 2, 2, -1, 1], [AA, AA, AA, AC, AC, AA, bad], [1, 1, 0, 1, -1, 0, 0])
    indptr, feature, molecules, reads, collapsed = ref.matrix()
    assert indptr == [0, 2, 2, 3]
    assert feature == [0, 1, 1]
    assert molecules == [1, 1, 1]
    assert reads == [1, 2, 1]
    assert collapsed == [1, 1, 1]
    assert ref.counts() == ([3, 0, 1], [2, 0, 1], 1, 0, 1)
    assert ref.n_no_feature == 1
    assert ref.total == 7
    assert [r[:4] for r in ref.pairs()] == [(0, 0, AA, 1), (0, 1, AA, 2), (2, 1, AC, 1)]


def test_same_umi_under_two_features_is_two_molecules():
    ref = M.FeatureMolecules(1, 4, 3, 2)
    ref.update([0, 0, 0], [umi3(G, T)] * 3, [3, 0, 3])
    assert ref.counts()[:2] == ([3], [2])
    assert ref.matrix() == ([0, 2], [0, 3], [1, 1], [1, 2], [1, 1])


def test_collapse_stays_inside_an_entry():
    """The header's AA x 1, AC x 2, GC x 5 chain under feature 0, and AA x 1, AC x 2 under feature 1 of
    the same barcode: the chains do not see each other."""
    AA, AC, GC = umi3(A, A), umi3(A, C), umi3(G, C)
    ref = M.FeatureMolecules(2, 2, 3, 2)
    index = [1] * 11
    umis = [AA] + [AC] * 2 + [GC] * 5 + [AA] + [AC] * 2
    features = [0] * 8 + [1] * 3
    ref.update(index, umis, features)
    indptr, feature, molecules, reads, collapsed = ref.matrix()
    assert (indptr, feature) == ([0, 0, 2], [0, 1])
    assert molecules == [3, 2] and reads == [8, 3]
    assert collapsed == [2, 1]  # AC and GC receive reads under feature 0; AC alone under feature 1
    assert ref.collapse() == ([0, 3], 3)
    assert ref.parent(1, 1, AC) == AC and ref.parent(1, 0, AC) == GC


def test_rule_order_and_range_errors():
    ref = M.FeatureMolecules(2, 3, 3, 1)  # feat_bits 2: feature 3 fits the bits and is out of range
    with pytest.raises(ValueError):
        ref.update([0, 0, 1, 1, 1], [A, A, A, N, N], [3, -3, 2, -1, 5])
    # the batch's other reads were counted: (1, 2, A); a bad UMI with no feature is a bad UMI (rule 4
    # before 4b); a bad UMI with a feature out of range is the range error (3b before 4)
    assert ref.counts() == ([0, 1], [0, 1], 0, 0, 1)
    assert ref.n_no_feature == 0 and ref.total == 5
    assert ref.matrix()[:3] == ([0, 0, 1], [2], [1])
    # -1 / -2 on the index come before anything about the feature
    ref.update([-1, -2], [A, A], [7, -9])
    assert ref.counts()[2:] == (1, 1, 1)


def test_row_sums_and_merge():
    a, b, whole = (M.FeatureMolecules(4, 5, 2, 3) for _ in range(3))
    reads = [((i * 7) % 4, (i * 3) % 5, (i * 11) % 64) for i in range(200)]
    for part, ref in ((reads[::2], a), (reads[1::2], b), (reads, whole)):
        ref.update([r[0] for r in part], [r[2] for r in part], [r[1] for r in part])
    # whole saw the reads in another order than a then b: the results do not depend on it
    a.merge(b)
    assert a.matrix() == whole.matrix() and a.counts() == whole.counts() and a.total == whole.total
    indptr, _, molecules, nreads, collapsed = whole.matrix()
    for i in range(4):
        lo, hi = indptr[i], indptr[i + 1]
        assert sum(molecules[lo:hi]) == whole.molecules[i]
        assert sum(nreads[lo:hi]) == whole.reads[i]
        assert sum(collapsed[lo:hi]) == whole.collapse()[0][i]


@pytest.mark.parametrize("nw, nf, kind, L, ok", [
    (737280, 8192, 3, 10, True),    # 20 + 13 + 30 = 63
    (737280, 8193, 3, 10, False),   # 14 feature bits
    (3_700_000, 2 ** 17, 2, 12, True),  # 22 + 17 + 24
    (3_700_000, 2 ** 17 + 1, 2, 12, False),
    (1, 1, 2, 30, True),            # 1 + 1 + 60
    (2, 2, 2, 31, False),           # 1 + 1 + 62
    (10, 0, 3, 4, False),
    (10, 2 ** 31, 2, 4, False),
])
def test_check_params(nw, nf, kind, L, ok):
    if ok:
        assert M.check_params(nw, nf, kind, L) == kind * L
    else:
        with pytest.raises(ValueError):
            M.check_params(nw, nf, kind, L)


def test_key_round_trip():
    for nw, nf, kind, L in ((3, 2, 3, 2), (737280, 8192, 3, 10), (1, 1, 2, 30)):
        umi = (1 << (kind * L)) - 1 if kind == 2 else int("100" * L, 2)
        k = M.key(nw - 1, nf - 1, umi, nf, kind, L)
        assert k < 2 ** 63
        assert M.unkey(k, nf, kind, L) == (nw - 1, nf - 1, umi)
